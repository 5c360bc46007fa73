"""GPU parity of the fused attention blocks at both widths (include/mxa.h mxa_cross_attention,
mxa_cross_attention_bits, mxa_qkv_attention_bits, mxa_attention_proj_bits; M.mx_cross_attention /
mx_qkv_attention / mx_topk_attention_proj with elem_bits 8 and 4): PixArt's MXCrossAttention.forward
and the self-attention block in one call each; elem_bits=4 is the reference's PixArt configuration.

The expected values come from the oracle chain of tests/cross_cases.py at the width: the exact
mx.Linears, the module's head split, the masked top-k attention core.  Bit-exact: the fp32
projections against the oracle; idx against the oracle; out and idx against M.mx_topk_attention
run on the device on those projections (the fused operands are what rows_prep / cols_prep, at width
4 attn_prep4_kernel, make of q, k, v); y against M.mx_linear and the oracle's Linear of the output
the device produced.  out against the oracle's: at width 8 normwise relative error <= 1e-3
 over the rows that are finite in the oracle; at width 4 row by row
(gpu_support.out_rows_close) at bfloat 0 / 32, at bfloat 16 against the unfused op alone.
tests/test_cross_cpu.py and tests/test_proj4_cpu.py (the width-4 caps) prove with the oracle alone that
the inputs sit in the regimes named here."""
import numpy as np
import pytest
import torch

import cross_cases as CC
from gpu_support import ELEM, OUT_TOL, M, dev, dev_opt, host, out_rows_close, same  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu
MODES = ("ex_pred", "MXINT4", "two_step_leading_ones")
BITS = pytest.mark.parametrize("bits", [8, 4])


def _out_close(out, r, vh, bits, what, bfloat=0):
    """out against the oracle's where it is finite there (module docstring)"""
    if bits == 8:
        fin = ~np.isnan(r["out"]).any(-1)
        err = O.normwise_rel_err(out[fin], r["out"][fin])
        print(f"{what}: out normwise error {err:.3e}")
        assert err <= OUT_TOL
    elif bfloat in (0, 32):
        out_rows_close(out, r, vh, what, bits=4)


def _check(M, bits, name, mode, flush, bfloat=0, with_bias=True, proj=True):
    """Every assertion of a main cross case (module docstring) on one parameter set."""
    (B, N, T, C, Ckv, H), k_top = CC.SHAPES[name]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, Wo, bo = CC.case(name)
    c = CC.chain(name, mode, flush, bfloat, with_bias, elem=ELEM[bits])
    r, bias = c["r"], dev_opt(c["bias"])
    kw = dict(k_top=k_top, pred_mode=mode, bias=bias, flush_subnormals=flush, bfloat=bfloat, elem_bits=bits)
    args = (dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5)
    out, idx, q, kv = M.mx_cross_attention(*args, return_proj=True, **kw)
    torch.cuda.synchronize()
    same(host(q), c["q"], "q projection vs oracle")
    same(host(kv), c["kv"], "kv projection vs oracle")
    same(host(idx), r["idx"], "idx vs oracle")
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, **kw)
    same(host(idx), host(i2), "idx vs the unfused op")
    same(host(out), host(o2), "out vs the unfused op")
    bad = np.isnan(r["out"]).any(-1)
    assert bad.sum() == H and bad[0, :, 3].all()  # test_cross_cpu / test_proj4_cpu: exactly the NaN token's rows
    same(np.isnan(host(out)).any(-1), bad, "NaN rows")
    _out_close(host(out), r, c["vh"], bits, f"{name} {mode}", bfloat)
    if not proj:
        return
    # ... and with to_out[0] behind it
    y, idx3 = M.mx_cross_attention(*args, proj_weight=dev(Wo), proj_bias=dev(bo), **kw)
    torch.cuda.synchronize()
    same(host(idx3), r["idx"], "idx with the proj")
    xo = out.transpose(1, 2).reshape(B, N, H * D)
    same(host(y), host(M.mx_linear(xo, dev(Wo), dev(bo), flush_subnormals=flush, bfloat=bfloat, elem_bits=bits)),
         "y vs mx_linear(out)")
    same(host(y), O.mx_linear(host(xo), Wo, bo, elem=ELEM[bits], flush=flush, bfloat=bfloat or 32), "y vs the oracle's Linear of out")


@BITS
@pytest.mark.parametrize("mode", MODES)
def test_cross_d48_ragged(M, mode, bits):
    """(3, 45, 70, 96, 160, 2), k = 20: D = 48 -- two 32-column blocks per head, D % 32 != 0 so
    the proj goes through the workspace copy; N and T ragged against 32, C != C_kv, T > N.  No
    flush: the PLAIN kernels (at width 4 rows_prep_block_plain4)."""
    _check(M, bits, "d48", mode, False)


@BITS
def test_cross_d32_one_wave(M, bits):
    """(2, 40, 20, 64, 64, 2), k = 7: D = 32 -- the Q workgroup is one wave; T < 32 (one partial
    token block), N > T.  PLAIN.  The proj's codes straight from the finishing kernel at width 8;
    at width 4 through the workspace copy although D % 32 == 0 (no MXINT4 codes out of it)."""
    _check(M, bits, "d32", "MXINT4", False)


@BITS
@pytest.mark.parametrize("mode", MODES)
def test_cross_d72_flush(M, mode, bits):
    """(2, 33, 77, 144, 96, 2), k = 20: D = 72, PixArt's head width; C no multiple of 64;
    flush_subnormals as PixArt runs: the general (non-PLAIN) kernels (at width 4 rows_prep_block<4>)."""
    _check(M, bits, "d72", mode, True)


@BITS
def test_cross_pixart_width(M, bits):
    """(1, 256, 120, 1152, 1152, 16), k = 20: the PixArt-alpha block, one image, with flush: 36
    K-blocks, the LDS size that decides the occupancy.  With the proj at width 8."""
    _check(M, bits, "pixart", "MXINT4", True, proj=bits == 8)


@BITS
def test_cross_bfloat16(M, bits):
    """bfloat = 16 on the first shape: the Linears' and the attention's bfloat rounding; at width 4
    with flush, the specification the reference's script runs."""
    _check(M, bits, "d48", "MXINT4", bits == 4, bfloat=16)


@BITS
def test_cross_without_bias(M, bits):
    _check(M, bits, "d48", "MXINT4", False, with_bias=False)


def test_cross4_tile_loads_where_used(M):
    """(1, 40, 33, 160, 160, 5), k = 7: the Q pass's 64 threads load 320 > 4 * 64 code chunks (not
    preloaded), the KV pass's 128 threads preload"""
    _check(M, 4, "d32w", "ex_pred", False)


@BITS
def test_cross_nan_in_cond(M, bits):
    """A NaN in one cond row of image 1 (cross_cases.nan_cond_case): idx equal to the oracle's,
    the same NaN pattern in out -- every row of that image -- and the other images finite."""
    H, x, cond, Wq, Wkv, q, kv, vh, r = CC.nan_cond_case(ELEM[bits])
    out, idx, qd, kvd = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), None, dev(Wkv), None, H, 32 ** -0.5, k_top=7,
                                             pred_mode="MXINT4", return_proj=True, elem_bits=bits)
    torch.cuda.synchronize()
    same(host(qd), q, "q")
    same(host(kvd), kv, "kv")
    same(host(idx), r["idx"], "idx")
    same(np.isnan(host(out)), np.isnan(r["out"]), "NaN pattern")
    assert np.isfinite(host(out)[[0, 2]]).all() and np.isnan(host(out)[1]).all()
    _out_close(host(out), r, vh, bits, "nan cond")


@BITS
def test_cross_dense_branch(M, bits):
    """top_k=False on the first shape (T <= 256: at width 4 finish_qk_kernel's MXINT4-P form): bit
    for bit the unfused op's dense branch on the same q, k, v, and the oracle's dense attention."""
    (B, N, T, C, Ckv, H), _ = CC.SHAPES["d48"]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, _, _ = CC.case("d48")
    c = CC.chain("d48", "MXINT4", False, 0, True, top_k=False, elem=ELEM[bits])
    bias = dev(c["bias"])
    out, idx, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5,
                                           top_k=False, bias=bias, return_proj=True, elem_bits=bits)
    torch.cuda.synchronize()
    assert idx is None
    same(host(q), c["q"], "q")
    same(host(kv), c["kv"], "kv")
    o2, _ = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, top_k=False, bias=bias, elem_bits=bits)
    same(host(out), host(o2), "dense out vs the unfused op")
    assert np.isnan(c["r"]["out"]).any(-1).sum() == H
    _out_close(host(out), c["r"], c["vh"], bits, "d48 dense")


# ---------------------------------------------------------------- self-attention
def _check_self(M, name, mode="ex_pred", flush=False, bfloat=0):
    (B, N, C, H), k = CC.SELF_SHAPES[name]
    D = C // H
    x, W, b, Wo, bo = CC.self_case(name)
    c = CC.self_chain(name, mode, flush, bfloat, "int4")
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
    same(host(y), O.mx_linear(host(xo), Wo, bo, elem="int4", flush=flush, bfloat=bfloat or 32), "y vs the oracle's int4 Linear of out")
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
@BITS
@pytest.mark.parametrize("H", [4, 2])
def test_cross_projection_spread_paths(M, H, bits):
    """The digit, shifted-int32 and fp64 accumulations of the Q and KV passes (at width 4 of the QKV
    pass too) in one launch each (cross_cases.spread_case / spread_case_qkv;
    test_cross_cpu.test_spread_case_paths names the path of every tile and head): the projections
    bit for bit the oracle's.  A wrong extent or stride of the one digit plane shows here."""
    elem = ELEM[bits]
    x, cond, Wq, bq, Wkv, bkv = CC.spread_case(H, elem)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), M.LinearWeightMX(dev(Wq), D, elem_bits=bits), dev(bq),
                                       M.LinearWeightMX(dev(Wkv), D, elem_bits=bits), dev(bkv), H, D ** -0.5, k_top=10,
                                       return_proj=True, elem_bits=bits)
    torch.cuda.synchronize()
    same(host(q), O.mx_linear(x, Wq, bq, elem=elem), "q across the accumulation paths")
    same(host(kv), O.mx_linear(cond, Wkv, bkv, elem=elem), "kv across the accumulation paths")
    if bits == 4:
        x, W, b = CC.spread_case_qkv(H, elem)
        _, _, qkv = M.mx_qkv_attention(dev(x), dev(W), dev(b), H, D ** -0.5, k_top=10, return_qkv=True, elem_bits=4)
        torch.cuda.synchronize()
        same(host(qkv), O.mx_linear(x, W, b, elem=elem), "qkv across the accumulation paths")


@BITS
@pytest.mark.parametrize("which", ["q", "kv"])
def test_cross_projection_digit_subnormal_gate(M, which, bits):
    """The digit path behind its subnormal gate in the Q pass (H = 4, a tiny bias) and in the KV
    pass (H = 2): cross_cases.subnormal_case, asserted in test_cross_cpu; at width 4 (run_f64 on the
    folded plane) in the QKV pass on the same scaled operands too."""
    elem = ELEM[bits]
    H, x, cond, Wq, bq, Wkv, bkv = CC.subnormal_case(which, elem)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev_opt(bq), dev(Wkv), dev_opt(bkv), H, D ** -0.5, k_top=10,
                                       return_proj=True, elem_bits=bits)
    torch.cuda.synchronize()
    same(host(q), O.mx_linear(x, Wq, bq, elem=elem), "q behind the subnormal gate")
    same(host(kv), O.mx_linear(cond, Wkv, bkv, elem=elem), "kv behind the subnormal gate")
    if bits == 4:
        tok, W = (x, np.concatenate([Wq, Wq, Wq])) if which == "q" else (cond, np.concatenate([Wkv[: Wkv.shape[0] // 2], Wkv]))
        _, _, qkv = M.mx_qkv_attention(dev(tok), dev(W), None, H, D ** -0.5, k_top=10, return_qkv=True, elem_bits=4)
        torch.cuda.synchronize()
        same(host(qkv), O.mx_linear(tok, W, elem=elem), "qkv behind the subnormal gate")


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


def test_cross_weight_headers_and_arguments(M):
    """A kv weight prepared with another group width, or other flush / bfloat settings, and a
    q weight of another in_features are refused; so is the proj without top-k."""
    rng = np.random.default_rng(9)
    B, N, T, C, H, D = 1, 40, 24, 64, 2, 32
    x, cond = dev(rng.standard_normal((B, N, C), dtype=np.float32)), dev(rng.standard_normal((B, T, C), dtype=np.float32))
    Wq = dev(rng.standard_normal((C, C), dtype=np.float32) * np.float32(0.05))
    Wkv = dev(rng.standard_normal((2 * C, C), dtype=np.float32) * np.float32(0.05))
    run = lambda wq, wkv, **kw: M.mx_cross_attention(x, cond, wq, None, wkv, None, H, D ** -0.5, k_top=8, **kw)  # noqa: E731
    out, idx = run(Wq, Wkv)
    o2, i2 = run(M.LinearWeightMX(Wq, D), M.LinearWeightMX(Wkv, D))
    same(host(out), host(o2), "prepared weights")
    with pytest.raises(ValueError):
        run(Wq, M.LinearWeightMX(Wkv, 2 * C))  # another group width
    with pytest.raises(ValueError):
        run(Wq, M.LinearWeightMX(Wkv, D, flush_subnormals=True))
    with pytest.raises(ValueError):
        run(Wq, M.LinearWeightMX(Wkv, D, bfloat=16))
    with pytest.raises(ValueError):
        run(dev(rng.standard_normal((C, 96), dtype=np.float32)), Wkv)  # in_features != C
    with pytest.raises(ValueError):
        run(Wq, Wkv, top_k=False, proj_weight=Wq)
    # past the Python checks: the library reads the header itself
    spoof = M.LinearWeightMX.__new__(M.LinearWeightMX)
    spoof.__dict__.update(M.LinearWeightMX(Wkv, D).__dict__)
    spoof.bfloat = 16  # the header says bfloat 0
    with pytest.raises(M.NativeError):
        run(Wq, spoof, bfloat=16)
    spoof.bfloat, spoof.group_width = 0, D
    spoof.buf = M.LinearWeightMX(Wkv, 2 * C).buf  # the header says one group of 2C columns
    with pytest.raises(M.NativeError):
        run(Wq, spoof)
