"""CPU checks of the cross-attention entry point (include/mxa.h mxa_cross_attention,
M.mx_cross_attention): the symbols, the argument validation that returns before any HIP call,
the workspace formula, the refusal of CPU tensors -- and, with the oracle alone, that the
inputs of tests/test_gpu_cross.py sit in the regimes those tests are about
(tests/cross_cases.py): the NaN rows at width 8, and at both widths every accumulation path in
every pass of the spread case and the digit tile behind its subnormal gate.  What exists at
width 4 only (the *_bits entry points' host logic, the eligible-share caps) is in
tests/test_proj4_cpu.py."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import cross_cases as CC
import gate_cases as GC
import gpu_support as GS
from oracle import mx_oracle as O

BITS = pytest.mark.parametrize("bits", [8, 4])


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native as N
    N.lib()
    return N


def _params(nat, B=8, H=16, Nq=256, T=120, D=72, k=20, C=1152, Ckv=1152):
    p = nat.AttnParams()
    p.out = 16  # non-null placeholders: validation launches nothing
    p.B, p.H, p.N, p.T, p.D, p.k_top = B, H, Nq, T, D, k
    p.pred_mode, p.top_k, p.approx, p.scale = nat.PRED_MODES["MXINT4"], 1, 1, D ** -0.5
    xc = nat.CrossParams()
    xc.x = xc.cond = xc.wq_q = xc.wq_kv = 16
    xc.C, xc.x_row_stride, xc.C_kv, xc.cond_row_stride = C, C, Ckv, Ckv
    return p, xc


def test_symbols_exported(nat):
    lib = nat.lib()
    for s in ("mxa_cross_attention", "mxa_cross_attention_workspace_bytes"):
        assert hasattr(lib, s) and s in nat.EXPORTS, s
    import mx_quantization_amd as M
    assert "mx_cross_attention" in M.__all__ and callable(M.mx_cross_attention)


def test_argument_validation_without_gpu(nat):
    """Every refusal here returns before the first HIP call (the prepared weights' headers are
    looked at only after the shape and settings checks)."""
    lib = nat.lib()
    p, xc = _params(nat)
    assert lib.mxa_cross_attention(None, None, None, None) == -1
    assert lib.mxa_cross_attention(ctypes.byref(p), None, None, None) == -1
    assert lib.mxa_cross_attention(None, ctypes.byref(xc), None, None) == -1
    assert lib.mxa_cross_attention_workspace_bytes(None, ctypes.byref(xc), None) == -1
    assert lib.mxa_cross_attention_workspace_bytes(ctypes.byref(p), None, None) == -1
    p, xc = _params(nat)
    xc.x_row_stride = xc.C - 1
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -1
    p, xc = _params(nat)
    xc.cond_row_stride = xc.C_kv - 1
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -1
    p, xc = _params(nat)
    xc.wq_kv = None
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -1
    p, xc = _params(nat, T=600)
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -2  # T > 512
    p, xc = _params(nat, D=160)
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -2  # D > 128
    for sdt in (nat.DT_F16, nat.DT_BF16):
        p, xc = _params(nat)
        p.score_dtype = sdt
        assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -2  # no autocast
    p, xc = _params(nat)
    p.out = None  # no output and no proj
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), None, None) == -1
    p, xc = _params(nat)
    p.top_k, p.k_top = 0, 0
    pj = nat.ProjParams()
    pj.wq = pj.y = 16
    pj.out_features = pj.y_row_stride = 1152
    assert lib.mxa_cross_attention(ctypes.byref(p), ctypes.byref(xc), ctypes.byref(pj), None) == -1  # proj: top-k only


def test_workspace_formula(nat):
    """The attention's workspace plus the MX codes and block exponents of both token sources,
    B*N x ceil(C/32) and B*T x ceil(C_kv/32) blocks; with pj the proj regions of
    mxa_attention_proj on top."""
    lib = nat.lib()
    for (B, H, Nq, T, D, C, Ckv) in [(8, 16, 256, 120, 72, 1152, 1152), (3, 2, 45, 70, 48, 96, 160), (2, 2, 40, 20, 32, 64, 64)]:
        p, xc = _params(nat, B, H, Nq, T, D, 7, C, Ckv)
        base = lib.mxa_attention_workspace_bytes(ctypes.byref(p))
        got = lib.mxa_cross_attention_workspace_bytes(ctypes.byref(p), ctypes.byref(xc), None)
        nbq, nbc = (C + 31) // 32, (Ckv + 31) // 32
        codes = B * Nq * nbq * 34 + B * T * nbc * 34
        assert base + codes <= got < base + codes + 4 * 256
        pj = nat.ProjParams()
        pj.out_features = C
        with_pj = lib.mxa_cross_attention_workspace_bytes(ctypes.byref(p), ctypes.byref(xc), ctypes.byref(pj))
        plain_pj = lib.mxa_attention_proj_workspace_bytes(ctypes.byref(p), None, ctypes.byref(pj))
        assert with_pj - got == plain_pj - base > 0
        hd = H * D
        want = (B * Nq + 31) // 32 * 32 * ((hd + 31) // 32) * 32 + B * Nq * ((hd + 31) // 32) * 2
        want += 0 if D % 32 == 0 else B * Nq * hd * 4  # the fp32 copy when a 32-block of H*D spans two heads
        assert want <= with_pj - got < want + 3 * 256


def test_cpu_tensors_refused():
    import mx_quantization_amd as M
    x, cond = torch.zeros(1, 8, 64), torch.zeros(1, 6, 64)
    with pytest.raises(M.NativeError):
        M.mx_cross_attention(x, cond, torch.zeros(64, 64), None, torch.zeros(128, 64), None, 2, 0.125, k_top=4)


# ---------------------------------------------------------------- the regimes of the GPU tests' inputs
@pytest.mark.parametrize("name", ["d48", "d72"])
def test_nan_placement_in_the_oracle(name):
    """x[0, 3, 7] = NaN and a zero row in Wq: the oracle has exactly H NaN output rows -- query
    row 3 of image 0 in every head -- and every other row finite, so the GPU tests' tolerance
    check leaves out H of the B*H*N rows."""
    (B, N, T, C, Ckv, H), _ = CC.SHAPES[name]
    x, _, Wq, *_ = CC.case(name)
    assert np.isnan(x).sum() == 1 and np.isnan(x[0, 3, 7]) and (Wq[5] == 0).all()
    for flush, with_bias in ((name == "d72", True), (name == "d72", False)):
        c = CC.chain(name, "MXINT4", flush, 0, with_bias)
        assert np.isnan(c["q"]).any(-1).sum() == 1 and np.isnan(c["q"][0, 3]).all()
        assert not np.isnan(c["kv"]).any()
        bad = np.isnan(c["r"]["out"]).any(-1)
        assert bad.sum() == H and bad[0, :, 3].all()
        assert np.isfinite(c["r"]["out"][~bad]).all()


def test_nan_cond_in_the_oracle():
    """A NaN in one cond row of image 1: its key and value rows are NaN in every head, every
    output row of that image is NaN (the NaN score is the largest, torch.topk keeps it) and
    the other images are finite."""
    H, x, cond, Wq, Wkv, q, kv, _, r = CC.nan_cond_case()
    assert np.isnan(kv).any(-1).sum() == 1 and np.isnan(kv[1, 9]).all() and not np.isnan(q).any()
    bad = np.isnan(r["out"]).any(-1)
    assert bad[1].all() and not bad[0].any() and not bad[2].any()
    assert (r["idx"][1] == 9).any(-1).all()


# per width: the digit limit, the tiles' largest row spreads, one head's k column spread, the path counts
# (digit, int32, fp64) of the q, kv and qkv passes at H = 4 and 2 (asserted at width 4 only)
SPREADS = {8: (8, [8, 20, 9], 8, None),
           4: (4, [4, 20, 5], 4, {4: {"q": (6, 6, 12), "kv": (8, 8, 8), "qkv": (6, 6, 12)},
                                  2: {"q": (2, 2, 8), "kv": (4, 4, 4), "qkv": (2, 2, 8)}})}


@BITS
@pytest.mark.parametrize("H", [4, 2])
def test_spread_case_paths(H, bits):
    """Every pass of the spread case takes the digit, the shifted-int32 and the fp64 accumulation:
    tile 0 (row spreads at the digit limit, 8 / 4) digits for the heads whose columns spread within
    the limit and fp64 for the head spreading 10; tile 1 (row spreads 20) fp64; tile 2 (row spreads
    one above the limit, 9 / 5) shifted int32 sums where that + the column spread <= smax = 9 (at
    width 8: column spread 0), fp64 for the others."""
    elem, (limit, rows, kcol, want_counts) = GS.ELEM[bits], SPREADS[bits]
    x, cond, Wq, bq, Wkv, bkv = CC.spread_case(H, elem)
    assert CC.proj_smax(8) == 9
    hk = min(1, H - 1)
    passes = [("q", x, Wq, 1, {0: 10}), ("kv", cond, Wkv, 2, {hk: kcol})]
    if bits == 4:  # the QKV pass has a spread case at this width only
        xs, W3, _ = CC.spread_case_qkv(H, elem)
        passes.append(("qkv", xs, W3, 3, {0: 10, hk: 10 if hk == 0 else kcol}))
    counts = {}
    for what, tokens, W, parts, wide in passes:
        for b in range(tokens.shape[0]):
            _, smx, _ = GC.gemm_gate(tokens[b], W[:32], elem=elem)
            assert smx.tolist() == rows, smx
        for h in range(H):
            assert GC.row_stats(CC.head_rows(W, H, parts, h), False, elem=elem)[1].max() == wide.get(h, 0)
        paths = CC.spread_paths(tokens, W, H, parts, elem)  # (asserts the gate quantity >= -126 everywhere)
        for (b, tb, h), path in paths.items():
            sp = wide.get(h, 0)
            want = {0: "digit" if sp <= limit else "fp64", 1: "fp64", 2: "int32" if rows[2] + sp <= 9 else "fp64"}[tb]
            assert path == want, (what, b, tb, h, path)
        assert set(paths.values()) == {"digit", "int32", "fp64"}
        c = collections.Counter(paths.values())
        counts[what] = (c["digit"], c["int32"], c["fp64"])
    assert want_counts is None or counts == want_counts[H]
    assert 20 + 10 <= 34  # the widest span of scaled block exponents: exact in the fp64 sums


@BITS
@pytest.mark.parametrize("which", ["q", "kv"])
def test_subnormal_case_gate(which, bits):
    """The scaled pass's first tile: row and column spreads within the digit limit (the digit
    operands), the gate quantity at least 20 below -126 for every head, and more than 0.9 of the
    tile's results subnormal."""
    elem, limit = GS.ELEM[bits], SPREADS[bits][0]
    H, x, cond, Wq, bq, Wkv, bkv = CC.subnormal_case(which, elem)
    tokens, W, parts = (x, Wq, 1) if which == "q" else (cond, Wkv, 2)
    for h in range(H):
        Wh = CC.head_rows(W, H, parts, h)
        for b in range(tokens.shape[0]):
            q, smx, wsp = GC.gemm_gate(tokens[b, :32], Wh, elem=elem)
            assert smx[0] <= limit and wsp <= limit, (smx, wsp)
            assert q[0] <= GC.GATE - 20, q
    want = O.mx_linear(tokens, W, elem=elem)
    sub = np.isfinite(want) & (want != 0) & (np.abs(want) < GC.F32_MIN_NORMAL)
    assert sub[:, :32].mean() > 0.9
    if bits == 8:  # the other pass is unscaled: its results are normal
        other = O.mx_linear(cond, Wkv) if which == "q" else O.mx_linear(x, Wq)
        assert not (np.isfinite(other) & (other != 0) & (np.abs(other) < GC.F32_MIN_NORMAL)).any()
    else:  # the same gate in the QKV pass the GPU test builds from these operands
        W3 = np.concatenate([Wq, Wq, Wq]) if which == "q" else np.concatenate([Wkv[: Wkv.shape[0] // 2], Wkv])
        for h in range(H):
            q, smx, wsp = GC.gemm_gate(tokens[0, :32], CC.head_rows(W3, H, 3, h), elem=elem)
            assert smx[0] <= limit and wsp <= limit and q[0] <= GC.GATE - 20
