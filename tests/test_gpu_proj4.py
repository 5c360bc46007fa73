"""GPU parity of the W4A4 fused attention blocks (include/mxa.h mxa_qkv_attention_bits,
mxa_attention_proj_bits, mxa_cross_attention_bits; M.mx_qkv_attention / mx_topk_attention_proj /
mx_cross_attention with elem_bits=4): the reference's PixArt configuration in one call per block.

The expected values come from the oracle chain of tests/proj4_cases.py at elem="int4".  Bit-exact:
the fp32 projections against the oracle's int4 Linears; idx against the oracle; out and idx against
M.mx_topk_attention(.., elem_bits=4) run on the device on the oracle's projections (the fused
operands are what attn_prep4_kernel makes of q, k, v); y against M.mx_linear(.., elem_bits=4) and the
oracle's int4 Linear of the output the device produced.  out against the oracle row by row
(gpu_support.out_rows_close at bits=4) at bfloat 0 / 32; at bfloat 16 against the unfused op alone.
tests/test_proj4_cpu.py proves with the oracle alone that the inputs sit in the regimes named here."""
import ctypes

import numpy as np
import pytest
import torch

import cross_cases as CC
import proj4_cases as P
from gpu_support import M, dev, dev_opt, host, out_rows_close, same  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


def _check(M, name, mode, flush, bfloat=0, with_bias=True, proj=True):
    """Every assertion of a main cross case (module docstring) on one parameter set."""
    (B, N, T, C, Ckv, H), k_top = P.SHAPES[name]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, Wo, bo = P.case(name)
    c = P.chain(name, mode, flush, bfloat, with_bias)
    r, bias = c["r"], dev_opt(c["bias"])
    kw = dict(k_top=k_top, pred_mode=mode, bias=bias, flush_subnormals=flush, bfloat=bfloat)
    args = (dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5)
    out, idx, q, kv = M.mx_cross_attention(*args, return_proj=True, elem_bits=4, **kw)
    torch.cuda.synchronize()
    same(host(q), c["q"], "q projection vs the oracle's int4 Linear")
    same(host(kv), c["kv"], "kv projection vs the oracle's int4 Linear")
    same(host(idx), r["idx"], "idx vs oracle")
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, elem_bits=4, **kw)
    same(host(idx), host(i2), "idx vs the unfused op")
    same(host(out), host(o2), "out vs the unfused op")
    bad = np.isnan(r["out"]).any(-1)
    assert bad.sum() == H and bad[0, :, 3].all()  # test_proj4_cpu: exactly the NaN token's rows
    same(np.isnan(host(out)).any(-1), bad, "NaN rows")
    if bfloat in (0, 32):
        out_rows_close(host(out), r, c["vh"], f"{name} {mode}", bits=4)
    if not proj:
        return
    # ... and with to_out[0] behind it
    y, idx3 = M.mx_cross_attention(*args, proj_weight=dev(Wo), proj_bias=dev(bo), elem_bits=4, **kw)
    torch.cuda.synchronize()
    same(host(idx3), r["idx"], "idx with the proj")
    xo = out.transpose(1, 2).reshape(B, N, H * D)
    same(host(y), host(M.mx_linear(xo, dev(Wo), dev(bo), flush_subnormals=flush, bfloat=bfloat, elem_bits=4)),
         "y vs mx_linear(out, elem_bits=4)")
    same(host(y), P.lin4(host(xo), Wo, bo, flush, bfloat), "y vs the oracle's int4 Linear of out")


@pytest.mark.parametrize("mode", P.MODES)
def test_cross4_d48_ragged(M, mode):
    """(3, 45, 70, 96, 160, 2), k = 20: D % 32 != 0, ragged N and T, C != C_kv; rows_prep_block_plain4"""
    _check(M, "d48", mode, False)


def test_cross4_d32_one_wave(M):
    """(2, 40, 20, 64, 64, 2), k = 7: the Q pass one wave, T < 32; the proj through the workspace copy
    although D % 32 == 0 (no MXINT4 codes out of the finishing kernel)"""
    _check(M, "d32", "MXINT4", False)


@pytest.mark.parametrize("mode", P.MODES)
def test_cross4_d72_flush(M, mode):
    """(2, 33, 77, 144, 96, 2), k = 20, flush: rows_prep_block<4>"""
    _check(M, "d72", mode, True)


def test_cross4_bfloat16_flush(M):
    """bfloat = 16 and flush, the specification the reference's script runs"""
    _check(M, "d48", "MXINT4", True, bfloat=16)


def test_cross4_without_bias(M):
    _check(M, "d48", "MXINT4", False, with_bias=False)


def test_cross4_tile_loads_where_used(M):
    """(1, 40, 33, 160, 160, 5), k = 7: the Q pass's 64 threads load 320 > 4 * 64 code chunks (not
    preloaded), the KV pass's 128 threads preload"""
    _check(M, "d32w", "ex_pred", False)


def test_cross4_pixart_width(M):
    """(1, 256, 120, 1152, 1152, 16), k = 20: 36 K-blocks, the LDS size that decides the occupancy"""
    _check(M, "pixart", "MXINT4", True, proj=False)


def test_cross4_dense_branch(M):
    """top_k=False on d48 (T <= 256: finish_qk_kernel's MXINT4-P form)"""
    (B, N, T, C, Ckv, H), _ = P.SHAPES["d48"]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, _, _ = P.case("d48")
    c = P.chain("d48", "MXINT4", False, 0, True, False)
    bias = dev(c["bias"])
    out, idx, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5,
                                           top_k=False, bias=bias, return_proj=True, elem_bits=4)
    torch.cuda.synchronize()
    assert idx is None
    same(host(q), c["q"], "q")
    same(host(kv), c["kv"], "kv")
    o2, _ = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, top_k=False, bias=bias, elem_bits=4)
    same(host(out), host(o2), "dense out vs the unfused op")
    out_rows_close(host(out), c["r"], c["vh"], "d48 dense", bits=4)


def test_cross4_nan_in_cond(M):
    H, x, cond, Wq, Wkv, q, kv, vh, r = P.nan_cond_case()
    out, idx, qd, kvd = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), None, dev(Wkv), None, H, 32 ** -0.5, k_top=7,
                                             pred_mode="MXINT4", return_proj=True, elem_bits=4)
    torch.cuda.synchronize()
    same(host(qd), q, "q")
    same(host(kvd), kv, "kv")
    same(host(idx), r["idx"], "idx")
    assert np.isfinite(host(out)[[0, 2]]).all() and np.isnan(host(out)[1]).all()
    out_rows_close(host(out), r, vh, "nan cond", bits=4)


# ---------------------------------------------------------------- self-attention
def _check_self(M, name, mode="ex_pred", flush=False, bfloat=0):
    (B, N, C, H), k = P.SELF_SHAPES[name]
    D = C // H
    x, W, b, Wo, bo = P.self_case(name)
    c = P.self_chain(name, mode, flush, bfloat)
    r = c["r"]
    kw = dict(flush_subnormals=flush, bfloat=bfloat, **(dict(k_top=k, pred_mode=mode) if k else dict(top_k=False)))
    out, idx, qkv = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, return_qkv=True, elem_bits=4, **kw)
    torch.cuda.synchronize()
    same(host(qkv), c["qkv"], "qkv projection vs the oracle's int4 Linear")
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, elem_bits=4, **kw)
    same(host(out), host(o2), "out vs the unfused op")
    if k:
        same(host(idx), r["idx"], "idx vs oracle")
        same(host(idx), host(i2), "idx vs the unfused op")
    else:
        assert idx is None
    if bfloat in (0, 32):
        out_rows_close(host(out), r, c["vh"], f"self {name}", bits=4)
    if not k:
        return
    y, idx3 = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, proj_weight=dev(Wo), proj_bias=dev(bo),
                                 elem_bits=4, **kw)
    torch.cuda.synchronize()
    same(host(idx3), r["idx"], "idx with the proj")
    xo = out.transpose(1, 2).reshape(B, N, C)
    want = M.mx_linear(xo, dev(Wo), dev(bo), flush_subnormals=flush, bfloat=bfloat, elem_bits=4)
    same(host(y), host(want), "y vs mx_linear(out, elem_bits=4)")
    same(host(y), P.lin4(host(xo), Wo, bo, flush, bfloat), "y vs the oracle's int4 Linear of out")
    # the proj alone behind given q, k, v
    y2, idx4 = M.mx_topk_attention_proj(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, dev(Wo), dev(bo),
                                        elem_bits=4, **kw)
    same(host(idx4), r["idx"], "mx_topk_attention_proj idx")
    same(host(y2), host(want), "mx_topk_attention_proj y")


@pytest.mark.parametrize("name", ["d48", "d32", "d64k65", "d72dense"])
def test_self4(M, name):
    """(2, 45, 96, 2) k 20; (2, 40, 64, 2) k 7 -- D 32, also mx_topk_attention_proj's D % 32 == 0 workspace
    route; (1, 130, 128, 2) k 65 -- finish_qk_kernel behind the fused projection; (1, 77, 144, 2) dense"""
    _check_self(M, name)


def test_self4_d72_bfloat16_flush(M):
    """(1, 70, 144, 2), k = 20 at bfloat 16 + flush (mx_topk_attention_proj at D 72 included)"""
    _check_self(M, "d72", "MXINT4", True, 16)


# ---------------------------------------------------------------- the accumulation paths
@pytest.mark.parametrize("H", [4, 2])
def test_proj4_spread_paths(M, H):
    """The digit, shifted-int32 and fp64 accumulations of the Q, KV and QKV passes in one launch each
    (proj4_cases.spread_case / spread_case_qkv; test_proj4_cpu names every tile's path): the
    projections bit for bit the oracle's.  A wrong extent or stride of the one digit plane shows here."""
    x, cond, Wq, bq, Wkv, bkv = P.spread_case(H)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), M.LinearWeightMX(dev(Wq), D, elem_bits=4), dev(bq),
                                       M.LinearWeightMX(dev(Wkv), D, elem_bits=4), dev(bkv), H, D ** -0.5, k_top=10,
                                       return_proj=True, elem_bits=4)
    torch.cuda.synchronize()
    same(host(q), P.lin4(x, Wq, bq), "q across the accumulation paths")
    same(host(kv), P.lin4(cond, Wkv, bkv), "kv across the accumulation paths")
    x, W, b = P.spread_case_qkv(H)
    _, _, qkv = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, k_top=10, return_qkv=True, elem_bits=4)
    torch.cuda.synchronize()
    same(host(qkv), P.lin4(x, W, b), "qkv across the accumulation paths")


@pytest.mark.parametrize("which", ["q", "kv"])
def test_proj4_digit_subnormal_gate(M, which):
    """The one-digit tile behind its subnormal gate (run_f64 on the folded plane) in the Q and KV passes,
    and in the QKV pass on the same scaled operands"""
    H, x, cond, Wq, bq, Wkv, bkv = P.subnormal_case(which)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev_opt(bq), dev(Wkv), dev_opt(bkv), H, D ** -0.5,
                                       k_top=10, return_proj=True, elem_bits=4)
    torch.cuda.synchronize()
    same(host(q), P.lin4(x, Wq, bq), "q behind the subnormal gate")
    same(host(kv), P.lin4(cond, Wkv, bkv), "kv behind the subnormal gate")
    tok, W = (x, np.concatenate([Wq, Wq, Wq])) if which == "q" else (cond, np.concatenate([Wkv[: Wkv.shape[0] // 2], Wkv]))
    _, _, qkv = M.mx_qkv_attention(dev(tok), dev(W), None, H, D ** -0.5, k_top=10, return_qkv=True, elem_bits=4)
    torch.cuda.synchronize()
    same(host(qkv), P.lin4(tok, W), "qkv behind the subnormal gate")


# ---------------------------------------------------------------- refusals, siblings, workspace
def _small(M, bits=4):
    rng = np.random.default_rng(77)
    B, N, T, C, H = 1, 40, 24, 64, 2
    f = lambda *s, sc=1.0: dev(rng.standard_normal(s, dtype=np.float32) * np.float32(sc))  # noqa: E731
    return dict(x=f(B, N, C), cond=f(B, T, C), Wq=f(C, C, sc=0.05), Wkv=f(2 * C, C, sc=0.05), Wqkv=f(3 * C, C, sc=0.05),
                Wo=f(C, C, sc=0.05), H=H, D=C // H)


def test_refusals_at_width_4(M):
    s = _small(M)
    x, cond, H, D = s["x"], s["cond"], s["H"], s["D"]
    run = lambda wq, wkv, **kw: M.mx_cross_attention(x, cond, wq, None, wkv, None, H, D ** -0.5, k_top=8, elem_bits=4, **kw)  # noqa: E731
    run(s["Wq"], s["Wkv"])
    with pytest.raises(ValueError):  # an 8-bit prepared weight
        run(s["Wq"], M.LinearWeightMX(s["Wkv"], D))
    with pytest.raises(ValueError):
        run(s["Wq"], s["Wkv"], proj_weight=M.LinearWeightMX(s["Wo"], 64))
    with pytest.raises(ValueError):
        M.mx_qkv_attention(x, s["Wqkv"], None, H, D ** -0.5, k_top=8, autocast=torch.float16, elem_bits=4)
    with pytest.raises(ValueError):
        M.mx_qkv_attention(x, s["Wqkv"], None, H, D ** -0.5, k_top=8, elem_bits=5)
    with pytest.raises(M.NativeError, match=r"status -2\)"):  # ELSA
        M.mx_qkv_attention(x, s["Wqkv"], None, H, D ** -0.5, k_top=8, pred_mode="ELSA", elsa_proj=torch.eye(D, device="cuda"),
                           elem_bits=4)
    # mixed widths past the Python check: the library reads the headers itself
    spoof = M.LinearWeightMX.__new__(M.LinearWeightMX)
    spoof.__dict__.update(M.LinearWeightMX(s["Wkv"], D).__dict__)
    spoof.elem_bits = 4  # the header says MXINT8
    with pytest.raises(M.NativeError, match=r"status -1\)"):
        run(s["Wq"], spoof)
    spo = M.LinearWeightMX.__new__(M.LinearWeightMX)
    spo.__dict__.update(M.LinearWeightMX(s["Wo"], 64).__dict__)
    spo.elem_bits = 4
    with pytest.raises(M.NativeError, match=r"status -1\)"):
        run(s["Wq"], s["Wkv"], proj_weight=spo)
    # T = 513; (T 300, k 65)
    rng = np.random.default_rng(3)
    for T, k in ((513, 8), (300, 65)):
        c2 = dev(rng.standard_normal((1, T, 64), dtype=np.float32))
        with pytest.raises(M.NativeError, match=r"status -2\)"):
            M.mx_cross_attention(x, c2, s["Wq"], None, s["Wkv"], None, H, D ** -0.5, k_top=k, elem_bits=4)


def test_bits_8_is_the_sibling(M, monkeypatch):
    """mxa_cross_attention_bits(.., 8), mxa_qkv_attention_bits(.., 8) and mxa_attention_proj_bits(.., 8)
    through ctypes: out, idx and y byte for byte the siblings'"""
    s = _small(M)
    x, cond, H, D = s["x"], s["cond"], s["H"], s["D"]
    calls = {
        "cross": lambda: M.mx_cross_attention(x, cond, s["Wq"], None, s["Wkv"], None, H, D ** -0.5, k_top=8),
        "cross+proj": lambda: M.mx_cross_attention(x, cond, s["Wq"], None, s["Wkv"], None, H, D ** -0.5, k_top=8,
                                                   proj_weight=s["Wo"]),
        "qkv": lambda: M.mx_qkv_attention(x, s["Wqkv"], None, H, D ** -0.5, k_top=8),
        "qkv+proj": lambda: M.mx_qkv_attention(x, s["Wqkv"], None, H, D ** -0.5, k_top=8, proj_weight=s["Wo"]),
    }
    want = {n: [host(t) for t in f()] for n, f in calls.items()}
    lib, seen = M._native.lib(), []

    def bits8(name, bits):
        seen.append(name)
        return getattr(lib, name + "_bits_workspace_bytes"), getattr(lib, name + "_bits"), name + "_bits", (8,)
    monkeypatch.setattr(M.ops, "_fused_entry", bits8)
    for n, f in calls.items():
        for g, w in zip(f(), want[n]):
            g = host(g)
            assert g.tobytes() == w.tobytes(), n
    assert set(seen) == {"mxa_cross_attention", "mxa_qkv_attention", "mxa_attention_proj"}
    # ... and a 4-bit weight is MXA_ERR_ARG there too
    with pytest.raises(M.NativeError, match=r"status -1\)"):
        M.mx_cross_attention(x, cond, M.LinearWeightMX(s["Wq"], D, elem_bits=4), None, s["Wkv"], None, H, D ** -0.5, k_top=8)


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


def test_exact_workspace_at_width_4(M, monkeypatch):
    """each 4-bit entry point on a buffer of exactly its reported size: nothing past it, the same results"""
    s = _small(M)
    x, cond, H, D = s["x"], s["cond"], s["H"], s["D"]
    w4 = lambda w, g: M.LinearWeightMX(w, g, elem_bits=4)  # noqa: E731  (prepared outside the guarded calls)
    wq, wkv, wqkv, wo = w4(s["Wq"], D), w4(s["Wkv"], D), w4(s["Wqkv"], D), w4(s["Wo"], 64)
    rng = np.random.default_rng(8)
    q, k, v = (dev(rng.standard_normal((1, 2, 40, 72), dtype=np.float32)) for _ in range(3))
    wo72 = w4(dev(rng.standard_normal((96, 144), dtype=np.float32) * np.float32(0.05)), 96)
    kw = dict(k_top=8, elem_bits=4)
    calls = {
        "cross": lambda: M.mx_cross_attention(x, cond, wq, None, wkv, None, H, D ** -0.5, **kw),
        "cross+proj": lambda: M.mx_cross_attention(x, cond, wq, None, wkv, None, H, D ** -0.5, proj_weight=wo, **kw),
        "qkv": lambda: M.mx_qkv_attention(x, wqkv, None, H, D ** -0.5, **kw),
        "qkv+proj": lambda: M.mx_qkv_attention(x, wqkv, None, H, D ** -0.5, proj_weight=wo, **kw),
        "proj_d72": lambda: M.mx_topk_attention_proj(q, k, v, 72 ** -0.5, wo72, **kw),
    }
    roomy = {n: [host(t) for t in f()] for n, f in calls.items()}
    for n, f in calls.items():
        guard = _ExactWorkspace()
        monkeypatch.setattr(M.ops, "_workspace", guard)
        got = f()
        guard.check(n)
        for g, w in zip(got, roomy[n]):
            same(host(g), w, n + " exact vs roomy workspace")
