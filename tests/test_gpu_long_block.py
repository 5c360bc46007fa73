"""GPU parity of the self-attention block on rows of 513 .. 1,024 keys at both widths (include/mxa.h
mxa_qkv_attention_full, mxa_attention_proj_full; M.mx_qkv_attention and M.mx_topk_attention_proj with
more than 512 tokens): the qkv mx.Linear, the attention core and the proj mx.Linear in one call.

The expected values come from the oracle chain of tests/long_block_cases.py at the width.  Bit-exact:
the fp32 projection against the oracle's Linear; idx against the oracle; out and idx against
M.mx_topk_attention run on the device on the oracle's q, k, v (the fused operands are what the operand
builders make of q, k, v); y against M.mx_linear and the oracle's Linear of the output the device
produced -- whichever way the proj's input codes were made: by the 16-row finishing kernel itself (width
8, D % 32 == 0, k <= 32) or through the fp32 workspace copy and the row quantizer.  out against the
oracle's row by row (gpu_support.out_rows_close) at bfloat 0; tests/test_long_block_cpu.py proves with
the oracle alone that every case compared so is within the eligible-share caps."""
import ctypes

import numpy as np
import pytest
import torch

import long_block_cases as LB
from gpu_support import ELEM, M, dev, dev_opt, host, out_rows_close, same  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu
BITS = pytest.mark.parametrize("bits", [8, 4])


def _same_bytes(a, b, what):
    assert host(a).tobytes() == host(b).tobytes(), what


def _check(M, name, bits, mode="ex_pred", flush=False, bfloat=0, approx=True, masked=False):
    """Every assertion of a case (module docstring) on one parameter set."""
    (B, N, C, H), k, _ = LB.CASES[name]
    D = C // H
    x, W, b, Wo, bo = LB.case(name)
    c = LB.chain(name, mode, flush, bfloat, ELEM[bits], approx, masked)
    r, bias = c["r"], dev_opt(c["bias"])
    akw = dict(top_k=False) if not k else dict(k_top=k, **(dict(pred_mode=mode) if approx else dict(approx=False)))
    kw = dict(flush_subnormals=flush, bfloat=bfloat, elem_bits=bits, **akw)
    out, idx, qkv = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, return_qkv=True, attn_bias=bias, **kw)
    torch.cuda.synchronize()
    same(host(qkv), c["qkv"], "qkv projection vs the oracle's Linear")
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, bias=bias, **kw)
    _same_bytes(out, o2, "out vs the unfused op")
    if k:
        same(host(idx), r["idx"], "idx vs oracle")
        _same_bytes(idx, i2, "idx vs the unfused op")
    else:
        assert idx is None and i2 is None
    if bfloat in (0, 32):
        out_rows_close(host(out), r, c["vh"], f"{name} w{bits}", kernel=LB.kernel_of(k), bits=bits)
    if not k:
        return
    # ... and with the proj mx.Linear behind it
    y, idx3 = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, proj_weight=dev(Wo), proj_bias=dev(bo),
                                 attn_bias=bias, **kw)
    torch.cuda.synchronize()
    same(host(idx3), r["idx"], "idx with the proj")
    xo = out.transpose(1, 2).reshape(B, N, C)
    want = M.mx_linear(xo, dev(Wo), dev(bo), flush_subnormals=flush, bfloat=bfloat, elem_bits=bits)
    _same_bytes(y, want, "y vs mx_linear(out)")
    same(host(y), O.mx_linear(host(xo), Wo, bo, elem=ELEM[bits], flush=flush, bfloat=bfloat or 32),
         "y vs the oracle's Linear of out")
    # the proj alone behind given q, k, v
    pkw = {a: v for a, v in kw.items() if a != "top_k"}
    y2, idx4 = M.mx_topk_attention_proj(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, dev(Wo), dev(bo), bias=bias, **pkw)
    same(host(idx4), r["idx"], "mx_topk_attention_proj idx")
    _same_bytes(y2, want, "mx_topk_attention_proj y")


@BITS
@pytest.mark.parametrize("name", list(LB.CASES))
def test_long_block(M, name, bits):
    """each case of long_block_cases.CASES (its comment names what the case reaches), ex_pred, bfloat 0"""
    _check(M, name, bits)


@BITS
@pytest.mark.parametrize("mode", ["MXINT4", "two_step_leading_ones"])
def test_long_block_pred_modes(M, mode, bits):
    _check(M, "d32k20", bits, mode)


@BITS
def test_long_block_true_topk(M, bits):
    """approx=False: the selection ranks the true scores"""
    _check(M, "d32k20", bits, approx=False)


@BITS
def test_long_block_mask_bias(M, bits):
    """a (B, 1, N, N) attn_bias of 0 / -10000: the EXTRA instantiations, with the proj's codes too"""
    _check(M, "d32k20", bits, masked=True)


@BITS
def test_long_block_d72_bfloat16_flush(M, bits):
    """PixArt's settings at its head width: MXINT4, bfloat 16, flush (out against the unfused op only)"""
    _check(M, "d72k20", bits, "MXINT4", True, 16)


def test_long_block_d32_bfloat16_direct_codes(M):
    """bfloat 16 + flush on the direct-codes route (the XO epilogue's rounding and the flushed blocks)"""
    _check(M, "d32k20", 8, "MXINT4", True, 16)


def test_long_block_elsa(M):
    """ELSA (width 8 only) behind the fused projection on d64k30: the hashes and key norms are built from
    the operands the projection kernel wrote; idx the oracle's, out, idx and y the unfused ops'"""
    from mx_quantization_amd.funcs import _create_structured_orthogonal_matrix
    (B, N, C, H), k, _ = LB.CASES["d64k30"]
    D = C // H
    torch.manual_seed(D)
    proj = _create_structured_orthogonal_matrix(D).numpy()
    x, W, b, Wo, bo = LB.case("d64k30")
    c = LB.chain("d64k30")  # (the projection does not depend on the approximator)
    r = O.attention(c["qh"], c["kh"], c["vh"], D ** -0.5, k_top=k, pred_mode="ELSA", elsa_proj=proj)
    kw = dict(k_top=k, pred_mode="ELSA", elsa_proj=dev(proj))
    out, idx = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, **kw)
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, **kw)
    same(host(idx), r["idx"], "idx vs oracle")
    _same_bytes(idx, i2, "idx vs the unfused op")
    _same_bytes(out, o2, "out vs the unfused op")
    y, idx3 = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, proj_weight=dev(Wo), proj_bias=dev(bo), **kw)
    same(host(idx3), r["idx"], "idx with the proj")
    _same_bytes(y, M.mx_linear(out.transpose(1, 2).reshape(B, N, C), dev(Wo), dev(bo)), "y vs mx_linear(out)")


# ---------------------------------------------------------------- the workspace, the siblings, refusals
class _ExactWorkspace:
    """Stands in for ops._workspace: exactly the reported bytes, 4096 bytes of 0xA5 behind them"""

    def __init__(self):
        self.bufs = []

    def __call__(self, device, nbytes):
        assert nbytes > 0
        buf = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=device)
        self.bufs.append((buf, nbytes))
        return buf[:nbytes]

    def check(self, what):
        torch.cuda.synchronize()
        assert self.bufs, what
        for buf, nbytes in self.bufs:
            assert bool((buf[nbytes:] == 0xA5).all()), f"{what}: wrote past its {nbytes}-byte workspace"


@BITS
def test_exact_workspace(M, bits, monkeypatch):
    """each new entry point on a buffer of exactly its reported size: nothing past it, the same results;
    d32k20 the direct codes (width 8), d32k33 and d72k20 the copy, d64k129 the tiled MFMA kernel"""
    prep = lambda w, g: M.LinearWeightMX(dev(w), g, elem_bits=bits)  # noqa: E731  (prepared outside the guarded calls)
    calls = {}
    for name in ("d32k20", "d32k33", "d72k20", "d64k129", "d72dense"):
        (B, N, C, H), k, _ = LB.CASES[name]
        D = C // H
        x, W, b, Wo, bo = LB.case(name)
        xd, wq, bd = dev(x), prep(W, D), dev(b)
        kw = dict(elem_bits=bits, **(dict(k_top=k) if k else dict(top_k=False)))
        calls[name + " qkv"] = lambda xd=xd, wq=wq, bd=bd, H=H, D=D, kw=kw: M.mx_qkv_attention(xd, wq, bd, H, D ** -0.5, **kw)
        if k:
            wo, bod = prep(Wo, C), dev(bo)
            calls[name + " qkv+proj"] = lambda xd=xd, wq=wq, bd=bd, H=H, D=D, kw=kw, wo=wo, bod=bod: M.mx_qkv_attention(
                xd, wq, bd, H, D ** -0.5, proj_weight=wo, proj_bias=bod, **kw)
            c = LB.chain(name, elem=ELEM[bits])
            q, kk, v = dev(c["qh"]), dev(c["kh"]), dev(c["vh"])
            calls[name + " proj"] = lambda q=q, kk=kk, v=v, D=D, kw=kw, wo=wo, bod=bod: M.mx_topk_attention_proj(
                q, kk, v, D ** -0.5, wo, bod, **kw)
    for n, f in calls.items():
        roomy = [t if t is None else host(t) for t in f()]
        guard = _ExactWorkspace()
        with monkeypatch.context() as mp:
            mp.setattr(M.ops, "_workspace", guard)
            got = f()
            guard.check(n)
        for g, w in zip(got, roomy):
            assert (g is None) == (w is None)
            if g is not None:
                assert host(g).tobytes() == w.tobytes(), n + " exact vs roomy workspace"


@BITS
def test_short_rows_are_the_bits_siblings(M, bits, monkeypatch):
    """through ctypes at T = 70: mxa_qkv_attention_full and mxa_attention_proj_full write the bytes of
    their _bits siblings"""
    rng = np.random.default_rng(70)
    B, N, C, H = 1, 70, 64, 2
    D = C // H
    f = lambda *s, sc=1.0: dev(rng.standard_normal(s, dtype=np.float32) * np.float32(sc))  # noqa: E731
    x, Wqkv, Wo = f(B, N, C), f(3 * C, C, sc=0.05), f(C, C, sc=0.05)
    q, k, v = f(B, H, N, D), f(B, H, N, D), f(B, H, N, D)
    kw = dict(k_top=8, elem_bits=bits)
    calls = {
        "qkv": lambda: M.mx_qkv_attention(x, Wqkv, None, H, D ** -0.5, **kw),
        "qkv dense": lambda: M.mx_qkv_attention(x, Wqkv, None, H, D ** -0.5, top_k=False, elem_bits=bits),
        "qkv+proj": lambda: M.mx_qkv_attention(x, Wqkv, None, H, D ** -0.5, proj_weight=Wo, **kw),
        "proj": lambda: M.mx_topk_attention_proj(q, k, v, D ** -0.5, Wo, **kw),
    }
    lib, seen = M._native.lib(), []

    def bits_form(name, b):
        seen.append(name + "_bits")
        return getattr(lib, name + "_bits_workspace_bytes"), getattr(lib, name + "_bits"), name + "_bits", (b,)

    def full_form(name, b):
        seen.append(name + "_full")
        return getattr(lib, name + "_full_workspace_bytes"), getattr(lib, name + "_full"), name + "_full", (b,)
    monkeypatch.setattr(M.ops, "_fused_entry", bits_form)
    want = {n: [t if t is None else host(t) for t in fn()] for n, fn in calls.items()}
    monkeypatch.setattr(M.ops, "_fused_entry", full_form)
    for n, fn in calls.items():
        for g, w in zip(fn(), want[n]):
            assert (g is None) == (w is None)
            if g is not None:
                assert host(g).tobytes() == w.tobytes(), n
    assert set(seen) == {a + b for a in ("mxa_qkv_attention", "mxa_attention_proj") for b in ("_bits", "_full")}


def test_python_routes_by_row_length(M, monkeypatch):
    """up to 512 keys through _fused_entry (today's calls), over 512 the *_full entry points"""
    seen = []
    real = M.ops._fused_entry

    def spy(name, bits):
        seen.append((name, bits))
        return real(name, bits)
    monkeypatch.setattr(M.ops, "_fused_entry", spy)
    rng = np.random.default_rng(5)
    W = dev(rng.standard_normal((192, 64), dtype=np.float32) * np.float32(0.05))
    for N in (512, 513):
        x = dev(rng.standard_normal((1, N, 64), dtype=np.float32))
        for bits in (8, 4):
            M.mx_qkv_attention(x, W, None, 2, 32 ** -0.5, k_top=8, elem_bits=bits)
    torch.cuda.synchronize()
    assert seen == [("mxa_qkv_attention", 8), ("mxa_qkv_attention", 4)]


def test_long_rows_refuse_autocast_and_cross(M):
    (B, N, C, H), k, _ = LB.CASES["d32k20"]
    x, W, b, Wo, bo = LB.case("d32k20")
    with pytest.raises(M.NativeError, match=r"status -2\)"):
        M.mx_qkv_attention(dev(x), dev(W), dev(b), H, 32 ** -0.5, k_top=k, autocast=torch.float16)
    with pytest.raises(M.NativeError, match=r"status -2\)"):
        M.mx_qkv_attention(dev(x), dev(W), dev(b), H, 32 ** -0.5, k_top=k, autocast=torch.bfloat16)
    # cross-attention keeps T <= 512
    Wq, Wkv = dev(W[:C]), dev(W[C:])
    with pytest.raises(M.NativeError, match=r"status -2\)"):
        M.mx_cross_attention(dev(x[:, :40]), dev(x), Wq, None, Wkv, None, H, 32 ** -0.5, k_top=k)
    # ... and the existing entry points their 512 keys, called directly
    lib = M._native.lib()
    p, keep = M.ops._attn_shape_params(torch.device("cuda"), torch.float32, B, H, N, N, 32, 32 ** -0.5, k, "ex_pred", True,
                                       True, None, False, 0, None)
    wq = M.LinearWeightMX(dev(W), 32)
    xd = dev(x)
    out = torch.empty((B, H, N, 32), device="cuda")
    M.ops._bind_out(p, out)
    xp = M._native.QkvParams()
    xp.x, xp.x_row_stride, xp.C, xp.wq = xd.data_ptr(), C, C, wq.buf.data_ptr()
    ws = torch.empty(lib.mxa_qkv_attention_full_workspace_bytes(ctypes.byref(p), ctypes.byref(xp), 8), dtype=torch.uint8, device="cuda")
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    assert lib.mxa_qkv_attention(ctypes.byref(p), ctypes.byref(xp), None) == -2
    assert lib.mxa_qkv_attention_bits(ctypes.byref(p), ctypes.byref(xp), 8, None) == -2
    assert lib.mxa_qkv_attention_full(ctypes.byref(p), ctypes.byref(xp), 8, M._native.stream_ptr(torch.device("cuda"))) == 0
    torch.cuda.synchronize()
