"""GPU parity of cross-attention with its q and kv Linears fused in front (include/mxa.h
mxa_cross_attention, M.mx_cross_attention): PixArt's MXCrossAttention.forward in one call.

The expected values come from the oracle chain of tests/cross_cases.py: the two exact
mx.Linears, the module's head split, the masked top-k attention core.  Bit-exact: the fp32
projections against the oracle; idx against the oracle; out and idx against M.mx_topk_attention
run on the device on those projections (the fused operands are what rows_prep / cols_prep make
of q, k, v); y against M.mx_linear and the oracle's Linear of the output the device produced.
Tolerance: out against the oracle's, normwise relative error <= 1e-3 over
the rows that are finite in the oracle.  tests/test_cross_cpu.py proves with the oracle alone
that the inputs sit in the regimes named here."""
import numpy as np
import pytest
import torch

import cross_cases as CC
from gpu_support import OUT_TOL, M, dev, dev_opt, host, same  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu
MODES = ("ex_pred", "MXINT4", "two_step_leading_ones")


def _check(M, name, mode, flush, bfloat=0, with_bias=True):
    """Every assertion of a main case (module docstring) on one parameter set."""
    (B, N, T, C, Ckv, H), k_top = CC.SHAPES[name]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, Wo, bo = CC.case(name)
    c = CC.chain(name, mode, flush, bfloat, with_bias)
    r, bias = c["r"], dev_opt(c["bias"])
    kw = dict(k_top=k_top, pred_mode=mode, bias=bias, flush_subnormals=flush, bfloat=bfloat)
    args = (dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5)
    out, idx, q, kv = M.mx_cross_attention(*args, return_proj=True, **kw)
    torch.cuda.synchronize()
    same(host(q), c["q"], "q projection vs oracle")
    same(host(kv), c["kv"], "kv projection vs oracle")
    same(host(idx), r["idx"], "idx vs oracle")
    o2, i2 = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, **kw)
    same(host(idx), host(i2), "idx vs the unfused op")
    same(host(out), host(o2), "out vs the unfused op")
    fin = ~np.isnan(r["out"]).any(-1)
    assert (~fin).sum() == H and not fin[0, :, 3].any()  # test_cross_cpu: exactly the NaN token's rows
    err = O.normwise_rel_err(host(out)[fin], r["out"][fin])
    print(f"{name} {mode}: out normwise error {err:.3e}")
    assert err <= OUT_TOL
    same(np.isnan(host(out)).any(-1), ~fin, "NaN rows")
    # ... and with to_out[0] behind it
    y, idx3 = M.mx_cross_attention(*args, proj_weight=dev(Wo), proj_bias=dev(bo), **kw)
    torch.cuda.synchronize()
    same(host(idx3), r["idx"], "idx with the proj")
    xo = out.transpose(1, 2).reshape(B, N, H * D)
    same(host(y), host(M.mx_linear(xo, dev(Wo), dev(bo), flush_subnormals=flush, bfloat=bfloat)), "y vs mx_linear(out)")
    same(host(y), O.mx_linear(host(xo), Wo, bo, flush=flush, bfloat=bfloat or 32), "y vs the oracle's Linear of out")


@pytest.mark.parametrize("mode", MODES)
def test_cross_d48_ragged(M, mode):
    """(3, 45, 70, 96, 160, 2), k = 20: D = 48 -- two 32-column blocks per head, D % 32 != 0 so
    the proj goes through the workspace copy; N and T ragged against 32, C != C_kv, T > N.  No
    flush: the PLAIN kernels."""
    _check(M, "d48", mode, False)


def test_cross_d32_one_wave(M):
    """(2, 40, 20, 64, 64, 2), k = 7: D = 32 -- the Q workgroup is one wave; the proj's codes
    straight from the finishing kernel; T < 32 (one partial token block), N > T.  PLAIN."""
    _check(M, "d32", "MXINT4", False)


@pytest.mark.parametrize("mode", MODES)
def test_cross_d72_flush(M, mode):
    """(2, 33, 77, 144, 96, 2), k = 20: D = 72, PixArt's head width; C no multiple of 64;
    flush_subnormals as PixArt runs: the general (non-PLAIN) kernels."""
    _check(M, "d72", mode, True)


def test_cross_pixart_width(M):
    """(1, 256, 120, 1152, 1152, 16), k = 20: the PixArt-alpha block, one image, with flush."""
    _check(M, "pixart", "MXINT4", True)


def test_cross_bfloat16(M):
    """bfloat = 16 on the first shape: the Linears' and the attention's bfloat rounding."""
    _check(M, "d48", "MXINT4", False, bfloat=16)


def test_cross_without_bias(M):
    _check(M, "d48", "MXINT4", False, with_bias=False)


def test_cross_nan_in_cond(M):
    """A NaN in one cond row of image 1 (cross_cases.nan_cond_case): idx equal to the oracle's,
    the same NaN pattern in out -- every row of that image -- and the other images finite."""
    H, x, cond, Wq, Wkv, q, kv, r = CC.nan_cond_case()
    out, idx, qd, kvd = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), None, dev(Wkv), None, H, 32 ** -0.5, k_top=7,
                                             pred_mode="MXINT4", return_proj=True)
    torch.cuda.synchronize()
    same(host(qd), q, "q")
    same(host(kvd), kv, "kv")
    same(host(idx), r["idx"], "idx")
    same(np.isnan(host(out)), np.isnan(r["out"]), "NaN pattern")
    assert np.isfinite(host(out)[[0, 2]]).all() and np.isnan(host(out)[1]).all()
    assert O.normwise_rel_err(host(out)[[0, 2]], r["out"][[0, 2]]) <= OUT_TOL


def test_cross_dense_branch(M):
    """top_k=False on the first shape: bit for bit the unfused op's dense branch on the same
    q, k, v, and the oracle's dense attention within tolerance."""
    (B, N, T, C, Ckv, H), _ = CC.SHAPES["d48"]
    D = C // H
    x, cond, Wq, bq, Wkv, bkv, _, _ = CC.case("d48")
    c = CC.chain("d48", "MXINT4", False, 0, True, top_k=False)
    bias = dev(c["bias"])
    out, idx, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev(bq), dev(Wkv), dev(bkv), H, D ** -0.5,
                                           top_k=False, bias=bias, return_proj=True)
    torch.cuda.synchronize()
    assert idx is None
    same(host(q), c["q"], "q")
    same(host(kv), c["kv"], "kv")
    o2, _ = M.mx_topk_attention(dev(c["qh"]), dev(c["kh"]), dev(c["vh"]), D ** -0.5, top_k=False, bias=bias)
    same(host(out), host(o2), "dense out vs the unfused op")
    fin = ~np.isnan(c["r"]["out"]).any(-1)
    assert (~fin).sum() == H
    assert O.normwise_rel_err(host(out)[fin], c["r"]["out"][fin]) <= OUT_TOL


@pytest.mark.parametrize("H", [4, 2])
def test_cross_projection_spread_paths(M, H):
    """Both passes' three accumulations in one launch each (cross_cases.spread_case;
    test_cross_cpu.test_spread_case_paths names the path of every tile and head): q and kv bit
    for bit the oracle's."""
    x, cond, Wq, bq, Wkv, bkv = CC.spread_case(H)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), M.LinearWeightMX(dev(Wq), D), dev(bq),
                                       M.LinearWeightMX(dev(Wkv), D), dev(bkv), H, D ** -0.5, k_top=10,
                                       return_proj=True)
    torch.cuda.synchronize()
    same(host(q), O.mx_linear(x, Wq, bq), "q across the accumulation paths")
    same(host(kv), O.mx_linear(cond, Wkv, bkv), "kv across the accumulation paths")


@pytest.mark.parametrize("which", ["q", "kv"])
def test_cross_projection_digit_subnormal_gate(M, which):
    """The digit path behind its subnormal gate in the Q pass (H = 4, a tiny bias) and in the KV
    pass (H = 2): cross_cases.subnormal_case, asserted in test_cross_cpu."""
    H, x, cond, Wq, bq, Wkv, bkv = CC.subnormal_case(which)
    D = x.shape[-1] // H
    _, _, q, kv = M.mx_cross_attention(dev(x), dev(cond), dev(Wq), dev_opt(bq), dev(Wkv), dev_opt(bkv), H, D ** -0.5, k_top=10,
                                       return_proj=True)
    torch.cuda.synchronize()
    same(host(q), O.mx_linear(x, Wq, bq), "q behind the subnormal gate")
    same(host(kv), O.mx_linear(cond, Wkv, bkv), "kv behind the subnormal gate")


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
