"""The score bias through every stride the kernels read, and the output through a caller's strides
(tests/bias_cases.py: one smallest shape per finishing kernel and width; tests/test_bias_cases_cpu.py proves
from the oracle alone that each case runs on the kernel it names, that a wrong batch or head stride changes
every row's kept indices, and that the eligible shares of the row-wise bound stay within the caps).

The bias is real-valued on all of (B, H, N, T).  Its contiguous layout (a) is compared with the oracle
(the oracle's attention at the width): true, pred, idx and the mask bit for bit, out by the row-wise
bound.  The same values in other storage -- (b) every second element of a wider buffer, 4 bytes off 16-byte
alignment; (c) transposed storage; (d) rows padded by three elements -- must give the bytes of (a).  The
broadcast layouts (e) (H, N, T), (f) (1, H, 1, T), (g) (N, T) and the mask (h) are compared with the oracle on
the values they stand for.  Each with and without the scores (the EXTRA and plain instantiations; with a
bias finish16_kernel, finish_qk_kernel and finish_qk_long_kernel are EXTRA both times and finish_kernel reads
the bias unconditionally).

A caller's out: a (B, N, H, D + 3) buffer between guard elements, passed as buf[..., :D].permute(0, 2, 1, 3) --
every out stride non-default, rows unaligned -- receives the bytes of the default call and nothing else is
written.  What mx_topk_attention must refuse on the host is refused before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import bias_cases as BC
import cross_cases as CC
from gpu_support import M, attn_run, check_attn, check_siblings, dev, host, out_rows_close, r_kw, r_scale, same, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
ids = dict(ids=BC.case_id)
NAN = float("nan")


def stored(V, layout):
    """the device tensor V (B, H, N, T) in one of the storage layouts (a) .. (d); the unused elements are NaN"""
    B, H, N, T = V.shape
    if layout == "a":
        return V.contiguous()
    if layout == "c":
        return V.transpose(-1, -2).contiguous().transpose(-1, -2)
    buf = torch.full((B, H, N, 2 * T + 1 if layout == "b" else T + 3), NAN, dtype=V.dtype, device=V.device)
    view = buf[..., 1::2] if layout == "b" else buf[..., :T]
    view.copy_(V)
    return view


def test_layouts_have_the_strides_they_claim():
    V = dev(BC.inputs(BC.G16)[3])
    B, H, N, T = V.shape
    b, c, d = stored(V, "b"), stored(V, "c"), stored(V, "d")
    assert b.stride() == (H * N * (2 * T + 1), N * (2 * T + 1), 2 * T + 1, 2) and b.data_ptr() % 16 == 4
    assert c.stride() == (H * N * T, N * T, 1, N)
    assert d.stride() == (H * N * (T + 3), N * (T + 3), T + 3, 1)
    for t in (b, c, d):
        assert torch.equal(t, V)


def _run(M, c, bias, scores, **extra):
    q, k, v, _ = BC.inputs(c)
    return attn_run(M, q, k, v, r_scale(c), c.bits, scores, bias=bias, **r_kw(c), **extra)


def _same_bytes(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in got:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


def _against_oracle(got, c, vs, what):
    ref = BC.reference(c, vs)
    check_attn(got, ref, what, cmp=same_bits)
    out_rows_close(got["out"], ref, BC.inputs(c)[2], what, BC.KERNEL[c.kind], c.bits)


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_case_kind(M, c):
    """the finishing kernel of the call, bias bound (the query launches nothing)"""
    q, k, v, V = (dev(x) for x in BC.inputs(c))
    p, _, _, _ = M.ops._attn_params(q, k, v, r_scale(c), c.k, c.mode or "ex_pred", bool(c.k), bool(c.k) and c.mode is not None,
                                    V, False, 0, None)
    p.out = 16
    assert M._native.lib().mxa_attention_full_finish_kernel(ctypes.byref(p), c.bits) == c.kind


@pytest.mark.parametrize("scores", [True, False], ids=["scores", "plain"])
@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_bias_layouts(M, c, scores):
    V = dev(BC.inputs(c)[3])
    what = f"{BC.case_id(c)} scores={scores}"
    a = _run(M, c, stored(V, "a"), scores)
    _against_oracle(a, c, "full", what + " (a)")
    for layout in "bcd":
        _same_bytes(_run(M, c, stored(V, layout), scores), a, f"{what} ({layout}) vs (a)")
    for layout, vs in (("e", "hnt"), ("f", "h1t"), ("g", "nt"), ("h", "mask")):
        bias = BC.bias_values(c, vs)
        assert bias.ndim == {"e": 3, "f": 4, "g": 2, "h": 4}[layout]
        got = _run(M, c, bias, scores)
        _against_oracle(got, c, vs, f"{what} ({layout})")
        if layout == "h":  # the all -inf row of the last image, in every head
            assert np.isnan(got["out"][c.B - 1, :, 2]).all() and np.isnan(got["out"]).all(-1).sum() == c.H


@pytest.mark.parametrize("bits", [8, 4])
def test_scores_alone(M, bits):
    """mx_approx_scores with layouts (b) and (e): the oracle's pred bit for bit"""
    c = BC.G16._replace(bits=bits)
    q, k, _, V = (dev(x) for x in BC.inputs(c))
    for bias, vs in ((stored(V, "b"), "full"), (V[0].contiguous(), "hnt")):
        pred = M.mx_approx_scores(q, k, "ex_pred", bias=bias, elem_bits=bits)
        assert pred.dtype == torch.float32
        same_bits(host(pred), BC.reference(c, vs)["pred"], f"w{bits} pred, bias {vs}")


def test_sibling_entry_points(M):
    """every entry point that accepts the GATHER16 call, with layout (c): the bytes of mx_topk_attention"""
    q, k, v, V = (dev(x) for x in BC.inputs(BC.G16))
    check_siblings(M, q, k, v, r_scale(BC.G16), (8, 4), k_top=BC.G16.k, bias=stored(V, "c"))


# ---- the fused blocks ---------------------------------------------------------------------------------------
def _fused_checks(M, out, idx, r, heads, bias, scale, k_top, bits, what):
    same(host(idx), r["idx"], what + " idx vs the oracle")
    out_rows_close(host(out), r, heads[2], what, bits=bits)
    o2, i2 = M.mx_topk_attention(*(dev(t) for t in heads), scale, k_top=k_top, pred_mode="ex_pred", bias=bias, elem_bits=bits)
    same(host(idx), host(i2), what + " idx vs the unfused op")
    same_bits(host(out), host(o2), what + " out vs the unfused op")


@pytest.mark.parametrize("vs", ["full", "hnt"], ids=["a", "e"])
@pytest.mark.parametrize("bits", [8, 4])
def test_cross_attention_bias(M, bits, vs):
    (B, N, T, C, Ckv, H), k_top = CC.SHAPES["d48"]
    x, cond, Wq, bq, Wkv, bkv, _, _ = CC.case("d48")
    ch, bias, r = BC.cross_reference(bits, vs)
    bias, scale = dev(bias), (C // H) ** -0.5
    out, idx = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, scale, k_top=k_top,
                                    pred_mode="ex_pred", bias=bias, elem_bits=bits)
    torch.cuda.synchronize()
    _fused_checks(M, out, idx, r, (ch["qh"], ch["kh"], ch["vh"]), bias, scale, k_top, bits, f"cross d48 w{bits} {vs}")


@pytest.mark.parametrize("vs", ["full", "hnt"], ids=["a", "e"])
@pytest.mark.parametrize("bits", [8, 4])
def test_qkv_attention_bias(M, bits, vs):
    (B, N, C, H), k_top = CC.SELF_SHAPES["d48"]
    x, W, b, _, _ = CC.self_case("d48")
    qkv, heads, bias, r = BC.self_reference(bits, vs)
    bias, scale = dev(bias), (C // H) ** -0.5
    out, idx, got_qkv = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, scale, k_top=k_top, pred_mode="ex_pred", attn_bias=bias,
                                           elem_bits=bits, return_qkv=True)
    torch.cuda.synchronize()
    same(host(got_qkv), qkv, "the projection vs the oracle")
    _fused_checks(M, out, idx, r, heads, bias, scale, k_top, bits, f"self d48 w{bits} {vs}")


# ---- a caller's out -------------------------------------------------------------------------------------------
GUARD = 64
INT = {torch.float32: (torch.int32, 0x5A5A5A5A), torch.float16: (torch.int16, 0x5A5A), torch.bfloat16: (torch.int16, 0x5A5A)}


def _guarded_out(B, H, N, D, dtype):
    """(everything, the (B, H, N, D) view): a flat buffer filled with a sentinel pattern; behind GUARD + 1 elements
    (an odd offset: a 16-bit view is 2-byte aligned only) a (B, N, H, D + 3) block whose [..., :D] is the view"""
    n = B * N * H * (D + 3)
    flat = torch.empty(n + 2 * GUARD + 1, dtype=dtype, device="cuda")
    it, pat = INT[dtype]
    flat.view(it).fill_(pat)
    block = flat[GUARD + 1: GUARD + 1 + n].view(B, N, H, D + 3)
    return flat, block[..., :D].permute(0, 2, 1, 3)


def _check_callers_out(M, c, what, dtype=torch.float32, autocast=None):
    q, k, v, V = (dev(x).to(dtype) for x in BC.inputs(c))
    kw = dict(bias=V, return_mask=bool(c.k), elem_bits=c.bits, autocast=autocast, **r_kw(c))
    odt = autocast or dtype
    want = M.mx_topk_attention(q, k, v, r_scale(c), **kw)
    flat, view = _guarded_out(c.B, c.H, c.N, c.D, odt)
    assert view.stride() == (c.N * c.H * (c.D + 3), c.D + 3, c.H * (c.D + 3), 1)
    assert view.data_ptr() % 4 == (0 if odt == torch.float32 else 2)
    got = M.mx_topk_attention(q, k, v, r_scale(c), out=view, **kw)
    torch.cuda.synchronize()
    it, pat = INT[odt]
    assert got[0] is view and want[0].dtype == odt and want[0].is_contiguous()
    assert torch.equal(view.contiguous().view(it), want[0].view(it)), what + ": out differs from the default call's"
    # everything outside the view still holds the sentinel
    keep = torch.ones(flat.shape, dtype=torch.bool, device="cuda")
    n = c.B * c.N * c.H * (c.D + 3)
    keep[GUARD + 1: GUARD + 1 + n].view(c.B, c.N, c.H, c.D + 3)[..., :c.D] = False
    assert bool((flat.view(it)[keep] == pat).all()), what + ": an element outside the view was written"
    assert not bool((view.contiguous().view(it) == pat).all())
    if c.k:
        assert torch.equal(got[1], want[1]) and torch.equal(got[-1], want[-1]), what + ": idx / mask"
    else:
        assert got[1] is None


@pytest.mark.parametrize("c", BC.CASES, **ids)
def test_callers_out(M, c):
    _check_callers_out(M, c, BC.case_id(c))


@pytest.mark.parametrize("c", BC.XDT_CASES, **ids)
def test_callers_out_float16(M, c):
    """float16 q, k, v, bias and out: the XDT instantiations' 16-bit stores at odd element offsets"""
    _check_callers_out(M, c, BC.case_id(c) + " f16", torch.float16)


def test_callers_out_autocast_bfloat16(M):
    _check_callers_out(M, BC.G16, "g16 autocast bf16", autocast=torch.bfloat16)


# ---- refusals, on the host ---------------------------------------------------------------------------------
def test_refusals_before_any_launch(M):
    c = BC.G16
    q, k, v, V = (dev(x) for x in BC.inputs(c))
    B, H, N, D, T = c.B, c.H, c.N, c.D, c.T
    run = lambda **kw: M.mx_topk_attention(q, k, v, r_scale(c), k_top=c.k, **kw)  # noqa: E731
    new = lambda *shape, dtype=torch.float32, device="cuda": torch.empty(shape, dtype=dtype, device=device)  # noqa: E731
    for shape in ((B, H, N - 1, D), (B, H, N, D - 1), (B * H, N, D), (B, H, N, D + 1), (H, B, N, D)):
        with pytest.raises(ValueError):
            run(out=new(*shape))
    with pytest.raises(M.NativeError):
        run(out=new(B, H, N, D, device="cpu"))
    if torch.cuda.device_count() > 1:
        with pytest.raises(M.NativeError):
            run(out=new(B, H, N, D, device="cuda:1"))
    with pytest.raises(ValueError):
        run(out=new(B, H, N, 2 * D)[..., ::2])  # last stride 2
    with pytest.raises(TypeError):
        run(out=new(B, H, N, D, dtype=torch.float16))
    with pytest.raises(TypeError):
        run(out=new(B, H, N, D), autocast=torch.bfloat16)  # the call's out is bfloat16
    with pytest.raises(TypeError):
        run(bias=V.half())
    with pytest.raises(TypeError):
        run(bias=V.double())
    for shape in ((B, H, N, T + 1), (B, H + 1, N, T), (2, T), (B, H, N)):
        with pytest.raises((RuntimeError, ValueError)):
            run(bias=new(*shape))
    with pytest.raises((RuntimeError, ValueError)):
        M.mx_approx_scores(q, k, "ex_pred", bias=new(B, H, N, T + 1))
    with pytest.raises(M.NativeError):
        run(bias=V.cpu())
