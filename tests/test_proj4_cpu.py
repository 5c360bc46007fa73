"""CPU checks of the W4A4 fused blocks (include/mxa.h mxa_qkv_attention_bits, mxa_attention_proj_bits,
mxa_cross_attention_bits): the symbols, the validation that returns before any HIP call, the
workspace sizes -- and, with the oracle alone (tests/cross_cases.py at elem="int4"), the NaN rows and
the eligible-share caps of every width-4 output that tests/test_gpu_cross.py compares with the oracle
row by row.  The accumulation paths of the spread case and the subnormal gate are asserted at both
widths in tests/test_cross_cpu.py."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import attn4_cases as A4
import cross_cases as CC
import gpu_support as GS

UNSUPPORTED, ARG = -2, -1
NAMES = ("mxa_qkv_attention", "mxa_attention_proj", "mxa_cross_attention")
MODES = ("ex_pred", "MXINT4", "two_step_leading_ones")


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native as N
    N.lib()
    return N


def _params(nat, B=8, H=16, Nq=256, T=120, D=72, k=20, C=1152, Ckv=1152, mode="MXINT4"):
    """AttnParams, QkvParams, CrossParams, ProjParams with non-null placeholders: validation launches nothing"""
    p = GS.host_params(nat, B, H, Nq, T, D, k, mode)
    xq = nat.QkvParams()
    xq.x = xq.wq = 16
    xq.C, xq.x_row_stride = C, C
    xc = nat.CrossParams()
    xc.x = xc.cond = xc.wq_q = xc.wq_kv = 16
    xc.C, xc.x_row_stride, xc.C_kv, xc.cond_row_stride = C, C, Ckv, Ckv
    pj = nat.ProjParams()
    pj.wq = pj.y = 16
    pj.out_features = pj.y_row_stride = H * D
    return p, xq, xc, pj


def _calls(nat, p, xq, xc, pj, bits, with_pj=True):
    """the three entry points' statuses on these parameters (p.N == p.T for the first two)"""
    lib, r = nat.lib(), ctypes.byref
    res = {"cross": lib.mxa_cross_attention_bits(r(p), r(xc), r(pj) if with_pj else None, bits, None)}
    if p.N == p.T:
        res["qkv"] = lib.mxa_qkv_attention_bits(r(p), r(xq), bits, None)
        if with_pj:
            res["proj"] = lib.mxa_attention_proj_bits(r(p), r(xq), r(pj), bits, None)
    return res


def _sizes(nat, p, xq, xc, pj, bits, with_pj=True):
    lib, r = nat.lib(), ctypes.byref
    pjr = r(pj) if with_pj else None
    res = {"cross": lib.mxa_cross_attention_bits_workspace_bytes(r(p), r(xc), pjr, bits),
           "qkv": lib.mxa_qkv_attention_bits_workspace_bytes(r(p), r(xq), bits)}
    if with_pj:
        res["proj"] = lib.mxa_attention_proj_bits_workspace_bytes(r(p), r(xq), pjr, bits)
        res["proj_noxq"] = lib.mxa_attention_proj_bits_workspace_bytes(r(p), None, pjr, bits)
    return res


def test_symbols_exported_and_bound(nat):
    lib = nat.lib()
    for n in NAMES:
        for s in (n + "_bits", n + "_bits_workspace_bytes"):
            assert hasattr(lib, s) and s in nat.EXPORTS, s
            assert getattr(lib, s).restype is (nat.c_i64 if s.endswith("bytes") else nat.c_i32)
    assert lib.mxa_abi_version() == 6
    import inspect

    import mx_quantization_amd as M
    for f in (M.mx_qkv_attention, M.mx_topk_attention_proj, M.mx_cross_attention):
        assert inspect.signature(f).parameters["elem_bits"].default == 8


def test_other_widths(nat):
    p, xq, xc, pj = _params(nat, Nq=120)
    for bits in (5, 0, 16):
        assert set(_calls(nat, p, xq, xc, pj, bits).values()) == {ARG}, bits
        assert set(_sizes(nat, p, xq, xc, pj, bits).values()) == {-1}, bits
    lib = nat.lib()
    assert lib.mxa_qkv_attention_bits(ctypes.byref(p), None, 4, None) == ARG
    assert lib.mxa_attention_proj_bits(ctypes.byref(p), ctypes.byref(xq), None, 4, None) == ARG
    assert lib.mxa_cross_attention_bits(ctypes.byref(p), None, None, 4, None) == ARG


def test_refusals_at_width_4_without_gpu(nat):
    """each returns before the first HIP call (the prepared weights' headers come after)"""
    def statuses(with_pj=True, **change):
        kw = {k: v for k, v in change.items() if k in ("T", "Nq", "k", "mode")}
        kw.setdefault("Nq", kw.get("T", 120))  # self-attention shapes, so that all three are called
        kw.setdefault("T", kw["Nq"])
        p, xq, xc, pj = _params(nat, **kw)
        for k, v in change.items():
            if k in ("score_dtype", "dtype", "top_k"):
                setattr(p, k, v)
            elif k == "autocast":
                xq.autocast_dtype = v
        if not p.top_k:
            p.k_top = 0
        return _calls(nat, p, xq, xc, pj, 4, with_pj)

    for sdt in (nat.DT_F16, nat.DT_BF16):
        assert set(statuses(score_dtype=sdt).values()) == {UNSUPPORTED}
        assert set(statuses(dtype=sdt).values()) == {UNSUPPORTED}
        got = statuses(autocast=sdt)
        assert got["qkv"] == got["proj"] == UNSUPPORTED
    assert set(statuses(mode="ELSA").values()) == {UNSUPPORTED}
    assert set(statuses(T=513).values()) == {UNSUPPORTED}
    assert set(statuses(T=300, k=65).values()) == {UNSUPPORTED}   # finish_kernel has no MXINT4-P form
    assert set(statuses(with_pj=False, T=300, top_k=0).values()) == {UNSUPPORTED}  # dense_rows_kernel
    # ... and what they accept reaches the header check (placeholder weights: MXA_ERR_ARG, no device needed)
    assert set(statuses().values()) == {ARG}
    assert set(statuses(T=256, k=65, with_pj=False).values()) == {ARG}
    assert set(statuses(with_pj=False, T=256, top_k=0).values()) == {ARG}


def test_workspace_sizes(nat):
    """(4) == (8) without pj and with pj at D = 72; with pj at D = 32 larger by the 256-byte-aligned fp32
    copy of the attention output"""
    for D, H in ((72, 16), (32, 4), (48, 2)):
        B, Nq = 2, 77
        p, xq, xc, pj = _params(nat, B, H, Nq, Nq, D, 7, H * D, 96)
        assert _sizes(nat, p, xq, xc, pj, 4, False) == _sizes(nat, p, xq, xc, pj, 8, False)
        s4, s8 = _sizes(nat, p, xq, xc, pj, 4), _sizes(nat, p, xq, xc, pj, 8)
        copy = (B * Nq * H * D * 4 + 255) // 256 * 256 if D % 32 == 0 else 0
        assert {n: s4[n] - s8[n] for n in s4} == {n: 0 if n == "qkv" else copy for n in s4}, D  # (qkv: no pj)


def test_bits_8_sizes_are_the_siblings(nat):
    lib, r = nat.lib(), ctypes.byref
    with open(os.path.join(GS.G, "host_table.json")) as f:
        shapes = json.load(f)["shapes"]
    for B, H, Nq, T, D, k in shapes:
        p, xq, xc, pj = _params(nat, B, H, Nq, T, D, k, H * D, H * D + 32)
        got = _sizes(nat, p, xq, xc, pj, 8)
        assert got["cross"] == lib.mxa_cross_attention_workspace_bytes(r(p), r(xc), r(pj))
        assert got["qkv"] == lib.mxa_qkv_attention_workspace_bytes(r(p), r(xq))
        assert got["proj"] == lib.mxa_attention_proj_workspace_bytes(r(p), r(xq), r(pj))
        assert got["proj_noxq"] == lib.mxa_attention_proj_workspace_bytes(r(p), None, r(pj))
        assert _sizes(nat, p, xq, xc, pj, 8, False)["cross"] == lib.mxa_cross_attention_workspace_bytes(r(p), r(xc), None)


def test_python_refusals_without_gpu():
    import mx_quantization_amd as M
    x = torch.zeros(1, 8, 64)
    with pytest.raises(ValueError):
        M.mx_qkv_attention(x, torch.zeros(192, 64), None, 2, 0.125, k_top=4, elem_bits=5)
    with pytest.raises(ValueError):
        M.mx_qkv_attention(x, torch.zeros(192, 64), None, 2, 0.125, k_top=4, elem_bits=4, autocast=torch.float16)
    with pytest.raises(M.NativeError):  # CPU tensors: no fallback at either width
        M.mx_cross_attention(x, x, torch.zeros(64, 64), None, torch.zeros(128, 64), None, 2, 0.125, k_top=4, elem_bits=4)


# ---------------------------------------------------------------- the eligible-share caps
CAPS = [(n, m, f) for n in ("d48", "d32", "d72") for m in MODES for f in (False, True)] + [("d32w", "ex_pred", False),
                                                                                              ("pixart", "MXINT4", True)]


@pytest.mark.parametrize("name,mode,flush", CAPS, ids=[f"{n}-{m}-{'flush' if f else 'plain'}" for n, m, f in CAPS])
def test_output_caps_cross(name, mode, flush):
    """the eligible shares of every cross case compared by out_rows_close, from the oracle alone; exactly
    H NaN rows -- the NaN token's"""
    H = CC.SHAPES[name][0][5]
    c = CC.chain(name, mode, flush, elem="int4")
    ok, (se, sr) = A4.shares_within_caps(c["r"], c["vh"])
    assert ok and se == 0 and sr == 0, (se, sr)
    bad = np.isnan(c["r"]["out"]).any(-1)
    assert bad.sum() == H and bad[0, :, 3].all()
    assert np.isnan(c["q"]).any(-1).sum() == 1 and not np.isnan(c["kv"]).any()


def test_output_caps_other_cases():
    c = CC.chain("d48", "MXINT4", False, 0, True, False, elem="int4")  # dense
    assert A4.shares_within_caps(c["r"], c["vh"])[1] == (0, 0)
    assert np.isnan(c["r"]["out"]).any(-1).sum() == 2
    c = CC.chain("d48", "MXINT4", False, 0, False, elem="int4")  # without the mask bias
    assert A4.shares_within_caps(c["r"], c["vh"])[1] == (0, 0)
    for name in ("d48", "d32", "d64k65", "d72dense"):
        c = CC.self_chain(name, elem="int4")
        assert A4.shares_within_caps(c["r"], c["vh"])[0], name
    H, x, cond, Wq, Wkv, q, kv, vh, r = CC.nan_cond_case("int4")
    assert A4.shares_within_caps(r, vh)[0]
    bad = np.isnan(r["out"]).any(-1)
    assert bad[1].all() and not bad[0].any() and not bad[2].any()

