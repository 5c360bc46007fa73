"""CPU checks of the self-attention block on rows of 513 .. 1,024 keys (include/mxa.h
mxa_qkv_attention_full, mxa_attention_proj_full): the symbols, the validation that returns before any HIP
call, the workspace sizes (the fp32 copy of the attention output exactly where the proj's codes are not
written directly), the siblings' answers on rows of at most 512 keys -- and, with the oracle alone
(tests/long_block_cases.py), the eligible-share caps of every output that tests/test_gpu_long_block.py
compares with the oracle row by row."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_support as GS
import long_block_cases as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, -1, -2
NEW = ("mxa_qkv_attention_full", "mxa_qkv_attention_full_workspace_bytes", "mxa_attention_proj_full",
       "mxa_attention_proj_full_workspace_bytes")


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native as N
    N.lib()
    return N


def _params(nat, B=1, H=2, N=513, D=32, k=20, mode="ex_pred", top_k=1, T=None):
    """AttnParams, QkvParams, ProjParams with non-null placeholders: validation launches nothing"""
    p = GS.host_params(nat, B, H, N, N if T is None else T, D, k if top_k else 0, mode, top_k)
    xq = nat.QkvParams()
    xq.x = xq.wq = 16
    xq.C = xq.x_row_stride = H * D
    pj = nat.ProjParams()
    pj.wq = pj.y = 16
    pj.out_features = pj.y_row_stride = H * D
    return p, xq, pj


def _full(nat, p, xq, pj, bits):
    """the statuses of the three forms: qkv, qkv + proj, proj behind given q, k, v"""
    lib, r = nat.lib(), ctypes.byref
    return {"qkv": lib.mxa_qkv_attention_full(r(p), r(xq), bits, None),
            "qkv+proj": lib.mxa_attention_proj_full(r(p), r(xq), r(pj), bits, None),
            "proj": lib.mxa_attention_proj_full(r(p), None, r(pj), bits, None)}


def _bits(nat, p, xq, pj, bits):
    lib, r = nat.lib(), ctypes.byref
    return {"qkv": lib.mxa_qkv_attention_bits(r(p), r(xq), bits, None),
            "qkv+proj": lib.mxa_attention_proj_bits(r(p), r(xq), r(pj), bits, None),
            "proj": lib.mxa_attention_proj_bits(r(p), None, r(pj), bits, None)}


def _full_sizes(nat, p, xq, pj, bits):
    lib, r = nat.lib(), ctypes.byref
    return {"qkv": lib.mxa_qkv_attention_full_workspace_bytes(r(p), r(xq), bits),
            "qkv+proj": lib.mxa_attention_proj_full_workspace_bytes(r(p), r(xq), r(pj), bits),
            "proj": lib.mxa_attention_proj_full_workspace_bytes(r(p), None, r(pj), bits)}


def _bits_sizes(nat, p, xq, pj, bits):
    lib, r = nat.lib(), ctypes.byref
    return {"qkv": lib.mxa_qkv_attention_bits_workspace_bytes(r(p), r(xq), bits),
            "qkv+proj": lib.mxa_attention_proj_bits_workspace_bytes(r(p), r(xq), r(pj), bits),
            "proj": lib.mxa_attention_proj_bits_workspace_bytes(r(p), None, r(pj), bits)}


# ---------------------------------------------------------------- the symbols
def test_symbols_in_header_bindings_and_library(nat):
    header = open(os.path.join(ROOT, "include", "mxa.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", nat.LIB_PATH], text=True)
    lib = nat.lib()
    for fn in NEW:
        assert re.search(r"\b" + fn + r"\s*\(", header), fn
        assert fn in nat._SIGS and fn in nat.EXPORTS and f" T {fn}\n" in syms, fn
        assert getattr(lib, fn).restype is (nat.c_i64 if fn.endswith("bytes") else nat.c_i32)
    assert lib.mxa_abi_version() == nat.ABI_VERSION == 6
    assert "#define MXA_ABI_VERSION 6" in header
    assert "MX_transformer_block.py:624-717" in open(os.path.join(ROOT, "include", "mxa.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for fn in NEW:
        assert f"_lib.{fn}.argtypes" in doc, fn


def test_python_signatures_unchanged():
    import inspect

    import mx_quantization_amd as M
    q = list(inspect.signature(M.mx_qkv_attention).parameters)
    assert q == ["x", "weight", "bias", "num_heads", "scale", "k_top", "pred_mode", "top_k", "approx", "flush_subnormals",
                 "bfloat", "return_qkv", "elsa_proj", "autocast", "proj_weight", "proj_bias", "elem_bits", "attn_bias"]
    t = list(inspect.signature(M.mx_topk_attention_proj).parameters)
    assert t == ["q", "k", "v", "scale", "proj_weight", "proj_bias", "k_top", "pred_mode", "approx", "bias",
                 "flush_subnormals", "bfloat", "elsa_proj", "elem_bits"]


# ---------------------------------------------------------------- refusals, before any HIP call
def test_null_structs_and_other_widths(nat):
    lib, r = nat.lib(), ctypes.byref
    p, xq, pj = _params(nat)
    assert lib.mxa_qkv_attention_full(r(p), None, 8, None) == ARG
    assert lib.mxa_attention_proj_full(r(p), r(xq), None, 8, None) == ARG
    assert lib.mxa_qkv_attention_full_workspace_bytes(r(p), None, 8) == -1
    assert lib.mxa_attention_proj_full_workspace_bytes(r(p), r(xq), None, 8) == -1
    for bits in (5, 0, 16):
        assert set(_full(nat, p, xq, pj, bits).values()) == {ARG}, bits
        assert set(_full_sizes(nat, p, xq, pj, bits).values()) == {-1}, bits


@pytest.mark.parametrize("bits", [8, 4])
def test_unchanged_answers(nat, bits):
    """pj with top_k == 0 and xq with N != T stay MXA_ERR_ARG, on long rows too"""
    p, xq, pj = _params(nat, top_k=0)
    got = _full(nat, p, xq, pj, bits)
    assert got["qkv+proj"] == got["proj"] == ARG
    p, xq, pj = _params(nat, N=600, T=513)
    got = _full(nat, p, xq, pj, bits)
    assert got["qkv"] == got["qkv+proj"] == ARG


@pytest.mark.parametrize("bits", [8, 4])
def test_refusals_on_long_rows(nat, bits):
    """MXA_ERR_UNSUPPORTED with placeholder pointers: nothing was launched, no header was read"""
    def statuses(**change):
        kw = {a: v for a, v in change.items() if a in ("N", "D", "mode")}
        p, xq, pj = _params(nat, **kw)
        for a, v in change.items():
            if a in ("dtype", "score_dtype"):
                setattr(p, a, v)
            elif a == "autocast":
                xq.autocast_dtype = v
        return _full(nat, p, xq, pj, bits)

    assert set(statuses(N=1025).values()) == {UNSUPPORTED}
    assert set(statuses(N=2048).values()) == {UNSUPPORTED}
    assert set(statuses(D=129).values()) == {UNSUPPORTED}
    for dt in (nat.DT_F16, nat.DT_BF16):
        for N in (513, 1024):
            assert set(statuses(N=N, dtype=dt).values()) == {UNSUPPORTED}
            assert set(statuses(N=N, score_dtype=dt).values()) == {UNSUPPORTED}
            got = statuses(N=N, autocast=dt)  # (the form without xq reads no autocast_dtype)
            assert got["qkv"] == got["qkv+proj"] == UNSUPPORTED
            got = statuses(N=N, autocast=dt, score_dtype=dt)
            assert set(got.values()) == {UNSUPPORTED}
    elsa = statuses(mode="ELSA")
    assert set(elsa.values()) == ({UNSUPPORTED} if bits == 4 else {ARG})  # (width 8: on to the header check)


@pytest.mark.parametrize("bits", [8, 4])
def test_existing_entry_points_keep_512(nat, bits):
    """mxa_qkv_attention, mxa_attention_proj and their _bits forms still refuse rows over 512 keys"""
    lib, r = nat.lib(), ctypes.byref
    for N in (513, 1024):
        p, xq, pj = _params(nat, N=N)
        assert set(_bits(nat, p, xq, pj, bits).values()) == {UNSUPPORTED}
        if bits == 8:
            assert lib.mxa_qkv_attention(r(p), r(xq), None) == UNSUPPORTED
            assert lib.mxa_attention_proj(r(p), r(xq), r(pj), None) == UNSUPPORTED
            assert lib.mxa_attention_proj(r(p), None, r(pj), None) == UNSUPPORTED
    xc = nat.CrossParams()
    xc.x = xc.cond = xc.wq_q = xc.wq_kv = 16
    xc.C = xc.x_row_stride = xc.C_kv = xc.cond_row_stride = 64
    p, xq, pj = _params(nat, N=40, T=513)
    assert lib.mxa_cross_attention_bits(r(p), r(xc), None, bits, None) == UNSUPPORTED


# ---------------------------------------------------------------- rows of at most 512 keys: the siblings
# test_proj4_cpu.py's shapes: its refusals' and its workspace sizes'
SHORT = [dict(N=120, D=72), dict(N=300, D=72, k=65), dict(N=300, D=72, top_k=0), dict(N=256, D=72, k=65),
         dict(N=256, D=72, top_k=0), dict(N=120, D=72, mode="ELSA"), dict(B=2, H=16, N=77, D=72, k=7),
         dict(B=2, H=4, N=77, D=32, k=7), dict(B=2, H=2, N=77, D=48, k=7), dict(N=512, D=64), dict(N=512, D=64, k=33),
         dict(N=512, D=128, k=65)]


@pytest.mark.parametrize("bits", [8, 4])
def test_short_rows_are_the_bits_siblings(nat, bits):
    for kw in SHORT:
        p, xq, pj = _params(nat, **kw)
        assert _full(nat, p, xq, pj, bits) == _bits(nat, p, xq, pj, bits), kw
        assert _full_sizes(nat, p, xq, pj, bits) == _bits_sizes(nat, p, xq, pj, bits), kw
        for a, v in (("dtype", nat.DT_F16), ("score_dtype", nat.DT_BF16)):
            p2, xq2, pj2 = _params(nat, **kw)
            setattr(p2, a, v)
            assert _full(nat, p2, xq2, pj2, bits) == _bits(nat, p2, xq2, pj2, bits), (kw, a)
        p2, xq2, pj2 = _params(nat, **kw)
        xq2.autocast_dtype = p2.score_dtype = nat.DT_F16
        assert _full(nat, p2, xq2, pj2, bits) == _bits(nat, p2, xq2, pj2, bits), (kw, "autocast")
    with_json = os.path.join(GS.G, "host_table.json")
    import json
    with open(with_json) as f:
        shapes = [s for s in json.load(f)["shapes"] if s[2] == s[3]]
    assert shapes
    for B, H, Nq, T, D, k in shapes:
        p, xq, pj = _params(nat, B, H, Nq, D, k)
        assert _full_sizes(nat, p, xq, pj, bits) == _bits_sizes(nat, p, xq, pj, bits), (B, H, Nq, D, k)


# ---------------------------------------------------------------- rows of 513 .. 1,024 keys
LONG_T, LONG_D, LONG_K = (513, 1000, 1024), (32, 64, 72, 128), (5, 20, 32, 33, 64, 65, 154)


@pytest.mark.parametrize("bits", [8, 4])
def test_long_rows_reach_the_header_check(nat, bits):
    """every k, at both widths, and the dense branch without pj: past every refusal, so the placeholder
    weights' header check answers (MXA_ERR_ARG; no device is needed for it)"""
    for T in LONG_T:
        for D in LONG_D:
            for k in LONG_K:
                for mode in ("ex_pred", "MXINT4", "two_step_leading_ones", "true_ex"):
                    p, xq, pj = _params(nat, N=T, D=D, k=k, mode=mode)
                    assert set(_full(nat, p, xq, pj, bits).values()) == {ARG}, (T, D, k, mode)
                p, xq, pj = _params(nat, N=T, D=D, k=k)
                p.approx = 0
                assert set(_full(nat, p, xq, pj, bits).values()) == {ARG}, (T, D, k, "approx=0")
            p, xq, pj = _params(nat, N=T, D=D, top_k=0)
            assert nat.lib().mxa_qkv_attention_full(ctypes.byref(p), ctypes.byref(xq), bits, None) == ARG, (T, D, "dense")


def test_long_rows_workspace_holds_the_copy_where_codes_are_not_direct(nat):
    """with pj the size is the attention's (mxa_attention_full's, plus x's MX rows with xq) plus the proj
    input's MX rows plus, exactly where the codes are not direct, the 256-byte-aligned fp32 copy"""
    lib, r = nat.lib(), ctypes.byref
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    seen = set()
    for B, H in ((1, 2), (2, 3)):
        for T in LONG_T:
            for D in LONG_D:
                for k in LONG_K:
                    p, xq, pj = _params(nat, B=B, H=H, N=T, D=D, k=k)
                    s = {bits: _full_sizes(nat, p, xq, pj, bits) for bits in (8, 4)}
                    core = lib.mxa_attention_full_workspace_bytes(r(p), 8)
                    assert core == lib.mxa_attention_full_workspace_bytes(r(p), 4) > 0
                    rows, cols = B * T, H * D
                    nb = (cols + 31) // 32
                    x_rows = al(rows * nb * 32) + al(rows * nb * 2)
                    y_rows = al((rows + 31) // 32 * 32 * nb * 32) + al(rows * nb * 2)
                    copy = al(rows * cols * 4)
                    for bits in (8, 4):
                        direct = LB.codes_direct(D, k, bits)
                        seen.add((bits, direct))
                        assert s[bits]["qkv"] == core + x_rows, (T, D, k, bits)
                        assert s[bits]["proj"] == core + y_rows + (0 if direct else copy), (T, D, k, bits)
                        assert s[bits]["qkv+proj"] == s[bits]["proj"] + x_rows, (T, D, k, bits)
                    # ... so the two widths differ by the copy where width 8 is direct, and nowhere else
                    d8 = LB.codes_direct(D, k, 8)
                    assert s[4]["proj"] - s[8]["proj"] == (copy if d8 else 0), (T, D, k)
                    assert d8 == (D % 32 == 0 and k <= 32)
    assert seen == {(8, True), (8, False), (4, False)}


def test_python_refuses_cpu_tensors_on_long_rows():
    import torch

    import mx_quantization_amd as M
    x = torch.zeros(1, 513, 64)
    with pytest.raises(M.NativeError):
        M.mx_qkv_attention(x, torch.zeros(192, 64), None, 2, 0.125, k_top=4)


# ---------------------------------------------------------------- the oracle's side of the GPU comparisons
# the shares the cases were chosen by (elements, rows), per width, from the oracle alone
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("name", list(LB.CASES))
def test_output_caps(name, bits):
    se, sr = LB.shares(name, bits)
    print(f"{name} w{bits}: eligible elements {se:.4%}, rows {sr:.2%}")
    assert se <= GS.ELIGIBLE_ELEMS and sr <= GS.ELIGIBLE_ROWS, (se, sr)
    c = LB.chain(name, elem=GS.ELEM[bits])
    assert np.isfinite(c["qkv"]).all() and np.isfinite(c["r"]["out"]).all()
    if LB.CASES[name].k:  # a kernel that read head 0's columns or keys for head 1 would show in idx
        idx = c["r"]["idx"]
        assert (idx[:, 0] != idx[:, 1]).any(-1).mean() > 0.9


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("kw", [dict(mode="MXINT4"), dict(mode="two_step_leading_ones"), dict(approx=False), dict(masked=True)],
                         ids=["MXINT4", "two_step_leading_ones", "trueK", "masked"])
def test_output_caps_of_the_d32k20_variants(kw, bits):
    se, sr = LB.shares("d32k20", bits, **kw)
    print(f"d32k20 {kw} w{bits}: eligible elements {se:.4%}, rows {sr:.2%}")
    assert se <= GS.ELIGIBLE_ELEMS and sr <= GS.ELIGIBLE_ROWS, (se, sr)
    if kw.get("masked"):  # every kept key is an unmasked one
        c = LB.chain("d32k20", elem=GS.ELEM[bits], masked=True)
        rows = np.arange(513)[None, None, :, None]
        assert ((c["r"]["idx"] + rows) % 2 == 0).all()
