"""GPU parity of the float16 / bfloat16 inputs and of torch.autocast, against vectors the
reference itself produced (tests/golden/gen_golden.py gen_dtype -> attn_dtype.npz; with a score
bias tests/golden/gen_dtype_bias_golden.py -> attn_dtype_bias*.npz, at the end of the file).

The reference's ops follow their input's dtype (microxscaling/mx/mx_ops.py:85, :283;
elemwise_ops.py:146): shared exponents are floor(log2) computed in the dtype, a float16
all-zero block quantizes to NaN, and the matmuls return the dtype.  Under torch.autocast
(deit engine.py:97) the fp32 q / k / v keep fp32 quantization but the matmuls return the
autocast dtype and P = zeros_like(true scores) is of it (deit main.py:101-152).

Bit-exact: MX values, shared exponents, true / approximate scores, top-k indices, the NaN
pattern of the output.  Tolerance: the output, normwise over its finite elements, within
the dtype's rounding (float16 1e-3, bfloat16 8e-3: the reference's P.V order is unpinned,
SURVEY.md F7, and bfloat16 carries 8 significant bits)."""
import functools
import os

import numpy as np
import pytest
import torch

import bias_cases as BC
import gpu_support
from gpu_support import TDT, G, M, from_bits, out_close, same, same_bits, to_bits, to_f32  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = {"f16": 1e-3, "bf16": 8e-3}
host = functools.partial(gpu_support.host, f32=True)  # every tensor here may be a 16-bit one


@pytest.fixture(scope="module")
def D():
    return np.load(os.path.join(G, "attn_dtype.npz"))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_shared_exponents_every_value(M, D, dt):
    """_shared_exponents(method='none') on every positive finite value of the dtype."""
    x = from_bits(D[f"{dt}/sexp_x"], dt)
    got = M.shared_exponents(x, "none")
    assert got.dtype == TDT[dt]
    same(host(got), D[f"{dt}/sexp_none"], f"{dt} floor(log2)")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_quantize_mx_kats(M, D, dt):
    """quantize_mx_op on dtype tensors: random blocks, the float16 zero-block NaN, tiny
    and large blocks, inf / NaN, both axes, int4, subnormal flush.  Bit patterns: the
    sign of a zero counts."""
    from mx_quantization_amd.mx import mx_ops
    from mx_quantization_amd.mx.specs import apply_mx_specs
    base = dict(block_size=32, scale_bits=8, shared_exp_method="max", custom_cuda=False,
                mx_flush_fp32_subnorms=False)
    x = from_bits(D[f"{dt}/q_x"], dt)
    s = apply_mx_specs(base)
    for key, fmt, ax, spec in (("q_int8_ax1", "int8", -1, s), ("q_int4_ax1", "int4", -1, s),
                               ("q_int8_ax0", "int8", -2, s),
                               ("q_int8_flush", "int8", -1, apply_mx_specs(dict(base, mx_flush_fp32_subnorms=True)))):
        got = mx_ops.quantize_mx_op(x, spec, elem_format=fmt, axes=[ax])
        assert got.dtype == TDT[dt]
        same_bits(host(got), D[f"{dt}/{key}"], f"{dt} {key}")
    if dt == "f16":  # the all-zero block of row 1 is NaN in float16 (0 / 2^-127 underflowed)
        assert np.isnan(D["f16/q_int8_ax1"][1, 32:64]).all()


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("tag,mode,k_top", [("deit", "ex_pred", 20), ("deit", "MXINT4", 20),
                                            ("deit", "partial_Q", 20), ("dit", "ex_pred", 154)])
def test_attention_dtype_inputs(M, D, dt, tag, mode, k_top):
    q, k, v = (from_bits(D[f"{dt}/{tag}/{n}"], dt) for n in "qkv")
    sc = q.shape[-1] ** -0.5
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, sc, k_top=k_top, pred_mode=mode, return_scores=True)
    assert out.dtype == TDT[dt]
    pre = f"{dt}/{tag}/{mode}"
    if f"{pre}/true" in D.files:
        same(host(true_s), to_f32(D[f"{pre}/true"], dt), pre + " true")
    if f"{pre}/pred" in D.files:
        same(host(pred_s), to_f32(D[f"{pre}/pred"], dt), pre + " pred")
    same(host(idx), D[f"{pre}/idx"].astype(np.int64), pre + " idx")
    out_close(host(out), to_f32(D[f"{pre}/out"], dt), TOL[dt], pre + " out")


def test_attention_dtype_finish32(M):
    """float16 inputs on the 32-row finishing kernel (its XDT instantiation: the dtype
    roundings at run time): k = 129 of T = 300 keys, N = 40 rows, D = 72, against the
    reference's own run (gen_golden.py gen_dtype_fin32 -> attn_dtype_fin32.npz)."""
    import ctypes
    F = np.load(os.path.join(G, "attn_dtype_fin32.npz"))
    q, k, v = (from_bits(F[f"f16/{n}"], "f16") for n in "qkv")
    k_top, sc = int(F["k_top"]), q.shape[-1] ** -0.5
    p, _, _, _ = M.ops._attn_params(q, k, v, sc, k_top, "ex_pred", True, True, None, False, 0, None)
    p.out = 16  # the query launches nothing
    assert M._native.lib().mxa_attention_finish_kernel(ctypes.byref(p)) == 2  # MXA_FIN_GATHER32
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, sc, k_top=k_top, return_scores=True)
    assert out.dtype == torch.float16
    pre = "f16/ex_pred"
    same(host(true_s), to_f32(F[f"{pre}/true"], "f16"), pre + " true")
    same(host(pred_s), to_f32(F[f"{pre}/pred"], "f16"), pre + " pred")
    same(host(idx), F[f"{pre}/idx"].astype(np.int64), pre + " idx")
    out_close(host(out), to_f32(F[f"{pre}/out"], "f16"), TOL["f16"], pre + " out")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("tag", ["deit", "dit"])
def test_attention_dtype_dense(M, D, dt, tag):
    q, k, v = (from_bits(D[f"{dt}/{tag}/{n}"], dt) for n in "qkv")
    out, _ = M.mx_topk_attention(q, k, v, q.shape[-1] ** -0.5, top_k=False)
    out_close(host(out), to_f32(D[f"{dt}/{tag}/dense/out"], dt), TOL[dt], f"{dt}/{tag} dense")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "dense"])
def test_attention_autocast(M, D, dt, mode):
    """fp32 q / k / v under torch.autocast: scores, P and out in the autocast dtype."""
    q, k, v = (torch.from_numpy(D[f"ac/{n}"]).cuda() for n in "qkv")
    pre = f"{dt}/ac/{mode}"
    if mode == "dense":
        out, _ = M.mx_topk_attention(q, k, v, 64 ** -0.5, top_k=False, autocast=TDT[dt])
        out_close(host(out), to_f32(D[f"{pre}/out"], dt), TOL[dt], pre)
        return
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, 64 ** -0.5, k_top=20, pred_mode=mode,
                                                   return_scores=True, autocast=TDT[dt])
    assert out.dtype == TDT[dt]
    if f"{pre}/true" in D.files:
        same(host(true_s), to_f32(D[f"{pre}/true"], dt), pre + " true")
        same(host(pred_s), to_f32(D[f"{pre}/pred"], dt), pre + " pred")
    same(host(idx), D[f"{pre}/idx"].astype(np.int64), pre + " idx")
    out_close(host(out), to_f32(D[f"{pre}/out"], dt), TOL[dt], pre + " out")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_qkv_attention_autocast_chain(M, D, dt):
    """mx.Linear qkv -> attention, both under torch.autocast, against the reference chain:
    projection bit-exact (fp32(dtype(x W^T)) + bias), idx bit-exact, out within tolerance."""
    x, W, b = (torch.from_numpy(D[f"acq/{n}"]).cuda() for n in ("x", "W", "bias"))
    out, idx, qkv = M.mx_qkv_attention(x, W, b, 3, 64 ** -0.5, k_top=20, pred_mode="ex_pred", return_qkv=True,
                                       autocast=TDT[dt])
    same(host(qkv), D[f"{dt}/acq/qkv"], f"{dt} autocast projection")
    same(host(idx), D[f"{dt}/acq/idx"].astype(np.int64), f"{dt} autocast chain idx")
    out_close(host(out), to_f32(D[f"{dt}/acq/out"], dt), TOL[dt], f"{dt} autocast chain out")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_mx_matmul_dtype(M, D, dt):
    from mx_quantization_amd.mx import matmul
    from mx_quantization_amd.mx.specs import apply_mx_specs
    s = apply_mx_specs(dict(block_size=32, scale_bits=8, shared_exp_method="max", custom_cuda=False,
                            a_elem_format="int8", w_elem_format="int8"))
    a, b = from_bits(D[f"{dt}/mm_a"], dt), from_bits(D[f"{dt}/mm_b"], dt)
    c = matmul(a, b, mx_specs=s, mode_config="aa")
    assert c.dtype == TDT[dt]
    out_close(host(c), D[f"{dt}/mm_c"], TOL[dt], f"{dt} mx.matmul")


def test_elsa_rejects_bias(M):
    """ELSA scores carry no bias in the reference (deit main.py:120-121)."""
    q = torch.randn(1, 2, 64, 64, device="cuda")
    with pytest.raises(ValueError, match="ELSA"):
        M.mx_approx_scores(q, q, "ELSA", bias=torch.zeros(64, 64, device="cuda"),
                           elsa_proj=torch.eye(64, device="cuda"))


# ---- a score bias on 16-bit tensors and under autocast (gen_dtype_bias_golden.py) ---------------------------
# The reference's glue has `true_scores += bias` (in place: the sum stays in the scores' dtype) and
# `pred = pred + bias` (out of place: torch promotes a 16-bit autocast pred plus a float32 bias to float32).
# Inputs are stored once as float16 patterns; the bfloat16 tensors are their .to(bfloat16), the autocast
# case's float32 q, k, v their .float().
BIAS_SHAPES = {"g16": BC.G16, "mfma": BC.MFMA, "g32": BC.G32}


@pytest.fixture(scope="module")
def DB():
    files = [np.load(os.path.join(G, f"attn_dtype_bias{s}.npz")) for s in ("", "_g32", "_ac")]
    return {name: f[name] for f in files for name in f.files}


def _bias_inputs(DB, tag, dt):
    return tuple(from_bits(DB[f"{tag}/{n}"], "f16").to(TDT[dt]) for n in ("q", "k", "v", "bias"))


@pytest.mark.parametrize("dt,tag,mode", [(dt, tag, mode) for dt in ("f16", "bf16")
                                         for tag, mode in (("g16", "ex_pred"), ("g16", "MXINT4"), ("mfma", "ex_pred"), ("g32", "ex_pred"))
                                         if (dt, tag) != ("bf16", "g32")])
def test_attention_dtype_bias(M, DB, dt, tag, mode):
    """float16 / bfloat16 q, k, v and a real-valued (H, N, T) bias of the same dtype: the bias loads of the
    selection kernel and of the 16-bit (XDT) finishing kernels -- GATHER16, MFMA, GATHER32"""
    c = BIAS_SHAPES[tag]
    q, k, v, bias = _bias_inputs(DB, tag, dt)
    assert bias.shape == (c.H, c.N, c.T) and bias.dtype == TDT[dt]
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, c.D ** -0.5, k_top=c.k, pred_mode=mode, bias=bias, return_scores=True)
    assert out.dtype == TDT[dt]
    pre = f"{dt}/{tag}/{mode}"
    if tag == "g16":
        same_bits(host(true_s), to_f32(DB[f"{dt}/g16/true"], dt), pre + " true")
        same_bits(host(pred_s), to_f32(DB[f"{pre}/pred"], dt), pre + " pred")
        pred = M.mx_approx_scores(q, k, mode, bias=bias)
        assert pred.dtype == TDT[dt]
        same_bits(to_bits(pred), DB[f"{pre}/pred"], pre + " mx_approx_scores", dt=dt, patterns=True)
    same(host(idx), DB[f"{pre}/idx"].astype(np.int64), pre + " idx")
    out_close(host(out), to_f32(DB[f"{pre}/out"], dt), TOL[dt], pre + " out")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["dense_mfma", "dense_rows"])
def test_attention_dtype_bias_dense(M, DB, dt, kind):
    """the dense branch: DENSE_MFMA on the first two heads of the GATHER16 tensors, DENSE_ROWS on GATHER32's"""
    q, k, v, bias = _bias_inputs(DB, "g16" if kind == "dense_mfma" else "g32", dt)
    if kind == "dense_mfma":
        q, k, v, bias = q[:, :2], k[:, :2], v[:, :2], bias[:2]
    out, _ = M.mx_topk_attention(q, k, v, q.shape[-1] ** -0.5, top_k=False, bias=bias)
    out_close(host(out), to_f32(DB[f"{dt}/{kind}/out"], dt), TOL[dt], f"{dt} {kind}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("btag", ["real", "mask"])
def test_attention_autocast_bias(M, DB, dt, btag):
    """fp32 q / k / v and a float32 bias under torch.autocast: true = dtype(true + bias), pred the float32
    sum of the dtype's pred and the bias (tests/test_bias_cases_cpu.py: re-rounded, it ranks differently)"""
    c = BC.G16
    q, k, v = (t.float() for t in _bias_inputs(DB, "g16", "f16")[:3])
    bias = torch.from_numpy(DB[f"{btag}/bias"]).cuda()
    assert bias.dtype == torch.float32 and bias.shape == ((c.B, c.H, c.N, c.T) if btag == "real" else (c.B, 1, 1, c.T))
    pre = f"{dt}/{btag}"
    kw = dict(bias=bias, autocast=TDT[dt])
    out, idx, true_s, pred_s = M.mx_topk_attention(q, k, v, c.D ** -0.5, k_top=c.k, pred_mode="ex_pred", return_scores=True, **kw)
    assert out.dtype == TDT[dt] and DB[f"{pre}/pred"].dtype == np.float32
    same_bits(host(true_s), to_f32(DB[f"{pre}/true"], dt), pre + " true")
    same_bits(host(pred_s), DB[f"{pre}/pred"], pre + " pred")
    same(host(idx), DB[f"{pre}/idx"].astype(np.int64), pre + " idx")
    out_close(host(out), to_f32(DB[f"{pre}/out"], dt), TOL[dt], pre + " out")
    pred = M.mx_approx_scores(q, k, "ex_pred", **kw)
    assert pred.dtype == torch.float32
    same_bits(host(pred), DB[f"{pre}/pred"], pre + " mx_approx_scores")
    dense, _ = M.mx_topk_attention(q, k, v, c.D ** -0.5, top_k=False, **kw)
    out_close(host(dense), to_f32(DB[f"{pre}/dense/out"], dt), TOL[dt], pre + " dense out")
