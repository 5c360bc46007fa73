"""torch-facing wrappers over the C ABI.  torch only allocates and supplies the
stream; every byte of arithmetic happens in libmxa.so on the MI355X."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _native as N
from ._native import check, lib, require_device, stream_ptr

_WS: dict = {}
_ELSA_COS: dict = {}


def _workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    key = (device, stream_ptr(device))
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = buf
    return buf


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    return t


def _f32c(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    """None, or t as a contiguous float32 tensor (a bias, as the kernels read it)"""
    return None if t is None else _f32(t, name).contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dt(t: torch.Tensor, name: str) -> int:
    """MXA_DT_* of a float32 / float16 / bfloat16 tensor.  The kernels read the tensor in
    its own dtype and follow the reference's dtype rules (include/mxa.h MXA_DT_*)."""
    try:
        return N.DTYPES[t.dtype]
    except KeyError:
        raise TypeError(f"{name} must be float32, float16 or bfloat16 (got {t.dtype})") from None


def autocast_dtype(device_type: str = "cuda"):
    """torch.autocast's lower-precision dtype when it is enabled for `device_type`, else None."""
    if torch.is_autocast_enabled(device_type):
        return torch.get_autocast_dtype(device_type)
    return None


def _split(shape, axis):
    axis = axis % len(shape) if len(shape) else 0
    outer = 1
    for s in shape[:axis]:
        outer *= s
    inner = 1
    for s in shape[axis + 1:]:
        inner *= s
    return outer, (shape[axis] if len(shape) else 1), inner


def quantize_mx(A: torch.Tensor, elem_mbits: int = 8, block_size: int = 32, axis: int = -1, scale_bits: int = 8,
                round: str = "nearest", flush: bool = False, bfloat: int = 0, want_codes: bool = False):
    """MX block quantization along one axis (mx_ops.py:180-306).  Returns the
    dequantized tensor, plus (codes int8, block exponents int16) if want_codes."""
    dev = require_device(A)
    dt = _dt(A, "A")
    A = A.contiguous()
    y = torch.empty_like(A)
    outer, L, inner = _split(tuple(A.shape), axis)
    codes = exps = None
    if want_codes:
        bs = L if block_size == 0 else block_size
        codes = torch.empty(A.shape, dtype=torch.int8, device=dev)
        exps = torch.empty((outer, (L + bs - 1) // max(bs, 1), inner), dtype=torch.int16, device=dev)
    if A.numel():
        check(lib().mxa_quantize_mx(A.data_ptr(), y.data_ptr(), codes.data_ptr() if want_codes else None,
                                    exps.data_ptr() if want_codes else None, outer, L, inner, block_size,
                                    elem_mbits, scale_bits, N.ROUND_MODES[round], int(flush), int(bfloat), dt,
                                    stream_ptr(dev)), "mxa_quantize_mx")
    return (y, codes, exps) if want_codes else y


def shared_exponents(A: torch.Tensor, method: str = "max", axis: int = -1, block_size: int = 0,
                     ebits: int = 0) -> torch.Tensor:
    """_shared_exponents (mx_ops.py:49-99) for one axis; 'max' keeps the axis as
    the block count (size 1 when block_size covers the axis)."""
    dev = require_device(A)
    dt = _dt(A, "A")
    A = A.contiguous()
    outer, L, inner = _split(tuple(A.shape), axis)
    if method == "none":
        out = torch.empty_like(A)
        m = 1
    elif method == "max":
        bs = L if block_size == 0 else block_size
        shape = list(A.shape)
        shape[axis % A.dim()] = (L + bs - 1) // bs
        out = torch.empty(shape, dtype=A.dtype, device=dev)
        m = 0
    else:
        raise ValueError(f"Unrecognized shared exponent selection method {method}")
    if A.numel():
        check(lib().mxa_shared_exponents(A.data_ptr(), out.data_ptr(), outer, L, inner, block_size, m, ebits, dt,
                                         stream_ptr(dev)), "mxa_shared_exponents")
    return out


def quantize_bfloat(A: torch.Tensor, bfloat: int = 16, round: str = "nearest", allow_denorm: bool = True):
    """bfloatX elementwise quantization (elemwise_ops.py:201-216)."""
    dev = require_device(A)
    dt = _dt(A, "A")
    A = A.contiguous()
    y = torch.empty_like(A)
    if A.numel():
        check(lib().mxa_quantize_bfloat(A.data_ptr(), y.data_ptr(), A.numel(), int(bfloat), N.ROUND_MODES[round],
                                        int(allow_denorm), dt, stream_ptr(dev)), "mxa_quantize_bfloat")
    return y


OP_KINDS = {"sign": N.MXA_OP_SIGN, "mxint8": N.MXA_OP_MXINT8, "mxint4": N.MXA_OP_MXINT4,
            "exion": N.MXA_OP_EXION, "true_ex": N.MXA_OP_TRUE_EX}


def _elem_bits(elem_bits) -> int:
    """8 (MXINT8) or 4 (MXINT4); any other width is a ValueError"""
    if elem_bits not in (8, 4):
        raise ValueError(f"elem_bits must be 8 or 4 (got {elem_bits!r})")
    return int(elem_bits)


def approx_values(X: torch.Tensor, kind: str, flush: bool = False, bfloat: int = 0, elem_bits: int = 8) -> torch.Tensor:
    """Approximator operand values along the last axis (funcs/exponent_based_prediction.py).
    elem_bits: the width of the MX codes the values are derived from -- 8, or 4: the MXINT4
    MX_Q / MX_K of a_elem_format "int4" (include/mxa.h mxa_approx_values_bits)."""
    bits = _elem_bits(elem_bits)
    dev = require_device(X)
    dt = _dt(X, "X")
    X = X.contiguous()
    out = torch.empty_like(X)
    d = X.shape[-1]
    rows = X.numel() // d if d else 0
    if rows and bits == 8:
        check(lib().mxa_approx_values(X.data_ptr(), out.data_ptr(), rows, d, d, d, OP_KINDS[kind], int(flush),
                                      int(bfloat), dt, stream_ptr(dev)), "mxa_approx_values")
    elif rows:
        check(lib().mxa_approx_values_bits(X.data_ptr(), out.data_ptr(), rows, d, d, d, OP_KINDS[kind], int(flush),
                                           int(bfloat), dt, bits, stream_ptr(dev)), "mxa_approx_values_bits")
    return out


def topk(vals: torch.Tensor, k: int, return_mask: bool = False, packed: bool = True):
    """torch.topk(vals, k, dim=-1, largest=True, sorted=True) with torch's CPU
    index order (TopKImpl.h:45-86), computed on the device.  Returns (values, idx),
    plus the prune mask as packed words (..., ceil(n/32)) int32 if return_mask.

    packed (rows of <= 256 values): try the packed 32-bit pass first (mxa_topk_ws) -- the
    fast path for approximate scores, whose values leave the low mantissa byte free; rows
    that do not pack are redone by the 64-bit pass.  For arbitrary float rows (almost none
    pack) packed=False runs the 64-bit pass alone: DeiT-base-sized random rows 0.79 ms
    against 1.05 ms through the packed attempt (profiles/r06v1_ab_topk_fp32.txt)."""
    dev = require_device(vals)
    dt = _dt(vals, "vals")
    vals = vals.contiguous()
    n = vals.shape[-1]
    rows = vals.numel() // n if n else 0
    idx = torch.empty(vals.shape[:-1] + (k,), dtype=torch.int64, device=dev)
    out = torch.empty(vals.shape[:-1] + (k,), dtype=vals.dtype, device=dev)
    mask = torch.empty(vals.shape[:-1] + ((n + 31) // 32,), dtype=torch.int32, device=dev) if return_mask else None
    if rows:
        # the workspace path (rows of <= 256 values: the fused op's packed selection pass
        # and one-lane tail); 0 bytes: mxa_topk alone
        mp = mask.data_ptr() if return_mask else None
        if not packed:  # the 64-bit pass alone
            check(lib().mxa_topk(vals.data_ptr(), rows, n, n, k, idx.data_ptr(), out.data_ptr(), mp, dt,
                                 stream_ptr(dev)), "mxa_topk")
            return (out, idx, mask) if return_mask else (out, idx)
        wsb = lib().mxa_topk_workspace_bytes(rows, n, k)
        if wsb < 0:
            raise ValueError(f"topk: invalid shape rows={rows} n={n} k={k}")
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        check(lib().mxa_topk_ws(vals.data_ptr(), rows, n, n, k, idx.data_ptr(), out.data_ptr(), mp, dt, ws.data_ptr(),
                                wsb, stream_ptr(dev)), "mxa_topk")
    return (out, idx, mask) if return_mask else (out, idx)


def unpack_mask(words: torch.Tensor, n: int) -> torch.Tensor:
    """Packed prune-mask words (..., ceil(n/32)) -> bool (..., n) (bit j%32 of word j/32)."""
    bits = torch.arange(32, device=words.device, dtype=torch.int32)
    m = (words.unsqueeze(-1) >> bits) & 1
    return m.reshape(words.shape[:-1] + (-1,))[..., :n].bool()


def mx_matmul(a: torch.Tensor, b: torch.Tensor, elem_mbits_a: int = 8, elem_mbits_b: int = 8, flush: bool = False,
              bfloat: int = 0, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """MX matmul forward (matmul.py:31-100): a (..., M, K) along K, b (..., K, Nc) along K.
    Each operand is quantized in its own dtype; the product is rounded once to out_dtype
    (default: the operands' dtype, which must then agree -- torch.matmul's rule; under
    torch.autocast the caller passes the autocast dtype)."""
    dev = require_device(a, b)
    adt, bdt = _dt(a, "in1"), _dt(b, "in2")
    if out_dtype is None:
        if a.dtype != b.dtype:
            raise RuntimeError(f"expected both operands to have the same dtype, got {a.dtype} and {b.dtype}")
        out_dtype = a.dtype
    cdt = N.DTYPES[out_dtype]
    if a.dim() < 2 or b.dim() < 2:
        raise ValueError("mx matmul needs >= 2-D operands")
    batch_shape = torch.broadcast_shapes(a.shape[:-2], b.shape[:-2])
    M, K = a.shape[-2:]
    K2, Nc = b.shape[-2:]
    if K != K2:
        raise ValueError(f"inner dimensions differ: {K} vs {K2}")
    a = a.expand(batch_shape + (M, K)).contiguous()
    b = b.expand(batch_shape + (K, Nc))
    # b the transpose of a row-major (..., Nc, K) tensor (the callers' k.transpose(-2, -1)):
    # quantized from that layout along K (mxa_matmul_bt), no copy
    bt = b.transpose(-2, -1)
    transposed = bt.is_contiguous()
    if not transposed:
        b = b.contiguous()
    batch = 1
    for s in batch_shape:
        batch *= s
    c = torch.empty(batch_shape + (M, Nc), dtype=out_dtype, device=dev)
    if batch == 0 or M == 0 or Nc == 0:
        return c
    if K == 0:
        return c.zero_()
    nbytes = lib().mxa_matmul_workspace_bytes(batch, M, K, Nc)
    ws = _workspace(dev, nbytes)
    fn, bp = (lib().mxa_matmul_bt, bt.data_ptr()) if transposed else (lib().mxa_matmul, b.data_ptr())
    check(fn(a.data_ptr(), bp, c.data_ptr(), batch, M, K, Nc, M * K, K * Nc, elem_mbits_a, elem_mbits_b, int(flush),
             int(bfloat), adt, bdt, cdt, ws.data_ptr(), ws.numel(), stream_ptr(dev)), "mxa_matmul")
    return c


def _strides3(t: torch.Tensor, name: str):
    if t.dim() != 4:
        raise ValueError(f"{name} must be (B, H, rows, D)")
    if t.stride(3) != 1:
        raise ValueError(f"{name} must be contiguous in its last (head_dim) axis")
    return (t.stride(0), t.stride(1), t.stride(2))


def elsa_cos_table(d: int) -> torch.Tensor:
    """cos(clamp(pi/d * h - 0.127, 0)) for hamming distances h = 0..d, computed the way
    funcs/elsa_approximation.py:138-143 computes it (fp32 torch ops on the host, torch's
    CPU cosf).  A (d+1)-entry constant of the approximator; the per-pair scores are
    formed on the device."""
    h = torch.arange(d + 1, dtype=torch.float32)
    est = (torch.pi / d) * h
    return torch.cos(torch.clamp(est - 0.127, min=0))


def _attn_shape_params(dev, dtype, B, H, Nq, T, D, scale, k_top, pred_mode, top_k, approx, bias, flush_subnormals,
                       bfloat, elsa_proj, autocast=None):
    """(AttnParams, keep) of a call on (B, H, Nq, D) queries and T keys of torch dtype `dtype`:
    everything but q, k, v and the outputs (the fused projections produce q, k, v inside the
    call).  keep: tensors whose storage the call reads.  autocast: None, or the torch.autocast
    dtype (float16 / bfloat16) under which the reference's matmuls return that dtype
    (include/mxa.h score_dtype)."""
    sdt = 0
    if autocast is not None and autocast != torch.float32:
        if autocast not in (torch.float16, torch.bfloat16):
            raise TypeError(f"autocast dtype must be float16 or bfloat16 (got {autocast})")
        sdt = N.DTYPES[autocast]
    if approx and pred_mode == "ELSA" and bias is not None:
        # elsa_approximation.approximation_scores adds no bias (deit main.py:120-121, DiT
        # models.py:188-189, PixArt :676-677): ranking ELSA scores plus a bias would differ
        raise ValueError("pred_mode 'ELSA' takes no bias: the reference's ELSA scores are unbiased")
    if top_k and not (0 < k_top <= T):
        raise ValueError(f"k={k_top} out of range for {T} keys")
    if approx and pred_mode not in N.PRED_MODES:
        raise ValueError(f"pred_mode {pred_mode!r} not supported by the fused op "
                         f"(supported: {sorted(N.PRED_MODES)})")
    keep = []
    p = N.AttnParams()
    p.B, p.H, p.N, p.T, p.D = B, H, Nq, T, D
    p.k_top = int(k_top) if top_k else 0
    p.scale = float(torch.tensor(scale, dtype=torch.float32).item())  # torch: python scale -> fp32 operand
    p.pred_mode = N.PRED_MODES.get(pred_mode, 0)
    p.top_k, p.approx = int(bool(top_k)), int(bool(approx))
    p.flush_subnormals, p.bfloat = int(bool(flush_subnormals)), int(bfloat)
    p.dtype, p.score_dtype = N.DTYPES[dtype], sdt
    if bias is not None:
        if bias.dtype != dtype:
            raise TypeError(f"bias must have q's dtype {dtype} (got {bias.dtype})")
        bias4 = bias
        while bias4.dim() < 4:
            bias4 = bias4.unsqueeze(0)
        bias4 = bias4.expand(B, H, Nq, T)
        p.bias = bias4.data_ptr()
        p.bias_strides[:] = tuple(bias4.stride())
    if approx and pred_mode == "ELSA":
        if elsa_proj is None:
            raise ValueError("pred_mode 'ELSA' needs the caller's orthogonal matrix (elsa_proj)")
        if Nq != T:
            # elsa_approximation.py:142-143 broadcasts the key norms over the query rows
            raise RuntimeError(f"ELSA scores need N == T (got N={Nq}, T={T}): the reference's key-norm "
                               f"broadcast (funcs/elsa_approximation.py:142) fails otherwise")
        proj = _f32(elsa_proj, "elsa_proj").contiguous()
        if tuple(proj.shape) != (D, D):
            raise ValueError(f"elsa_proj must be ({D}, {D})")
        ck = (D, dev)
        if ck not in _ELSA_COS:
            _ELSA_COS[ck] = elsa_cos_table(D).to(dev)
        cos = _ELSA_COS[ck]
        keep += [proj, cos]
        p.elsa_proj, p.elsa_cos = proj.data_ptr(), cos.data_ptr()
    return p, keep


def _attn_params(q, k, v, scale, k_top, pred_mode, top_k, approx, bias, flush_subnormals, bfloat, elsa_proj,
                 autocast=None):
    """(AttnParams, device, (B, H, N, T, D), keep) for q, k, v tensors (v None: the scores alone)."""
    dev = require_device(q, k, v, bias, elsa_proj)
    _dt(q, "q")
    for t, nm in ((k, "k"),) + (((v, "v"),) if v is not None else ()):
        if t.dtype != q.dtype:
            raise TypeError(f"{nm} must have q's dtype {q.dtype} (got {t.dtype})")
    B, H, Nq, D = q.shape
    Bk, Hk, T, Dk = k.shape
    if (Bk, Hk, Dk) != (B, H, D) or (v is not None and tuple(v.shape) != (B, H, T, D)):
        raise ValueError(f"shape mismatch q{tuple(q.shape)} k{tuple(k.shape)} "
                         f"v{None if v is None else tuple(v.shape)}")
    p, keep = _attn_shape_params(dev, q.dtype, B, H, Nq, T, D, scale, k_top, pred_mode, top_k, approx, bias,
                                 flush_subnormals, bfloat, elsa_proj, autocast)
    p.q, p.k = q.data_ptr(), k.data_ptr()
    p.q_strides[:], p.k_strides[:] = _strides3(q, "q"), _strides3(k, "k")
    if v is not None:
        p.v = v.data_ptr()
        p.v_strides[:] = _strides3(v, "v")
    return p, dev, (B, H, Nq, T, D), keep


def _out_dtype(q, autocast):
    return autocast if autocast in (torch.float16, torch.bfloat16) else q.dtype


def _bind_out(p, out: torch.Tensor) -> torch.Tensor:
    p.out = out.data_ptr()
    p.out_strides[:] = (out.stride(0), out.stride(1), out.stride(2))
    return out


def _new_idx(p, B, H, Nq, k_top, top_k, dev):
    """The kept indices (B, H, N, k) int64 bound to p.idx_out; None without top-k."""
    idx = torch.empty((B, H, Nq, k_top), dtype=torch.int64, device=dev) if top_k else None
    p.idx_out = _ptr(idx)
    return idx


def _call_with_workspace(size_fn, fn, name, p, *extra, dev, bad="bad attention shape"):
    """fn(p, *extra, stream) on the stream's workspace of size_fn(p, *extra) bytes (extra: the
    call's further parameter structs by reference, or None).  bad: the ValueError's text for a
    negative size; None: no error here (fn refuses the call)."""
    nbytes = size_fn(ctypes.byref(p), *extra)
    if nbytes < 0 and bad is not None:
        raise ValueError(bad)
    ws = _workspace(dev, nbytes)
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel()
    check(fn(ctypes.byref(p), *extra, stream_ptr(dev)), name)


def mx_topk_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, k_top: int = 20,
                      pred_mode: str = "ex_pred", top_k: bool = True, approx: bool = True,
                      bias: Optional[torch.Tensor] = None, flush_subnormals: bool = False, bfloat: int = 0,
                      return_scores: bool = False, out: Optional[torch.Tensor] = None,
                      return_mask: bool = False, elsa_proj: Optional[torch.Tensor] = None,
                      autocast: Optional[torch.dtype] = None, elem_bits: int = 8):
    """The fused hot path (include/mxa.h mxa_attention_full): q (B,H,N,D), k/v (B,H,T,D)
    float32, float16 or bfloat16 (strided views of a packed qkv are fine; the ops follow
    the tensors' dtype as the reference's do).  autocast: the torch.autocast dtype the
    reference's matmuls would return (scores, P and out in it).  Returns (out (B,H,N,D),
    idx (B,H,N,k_top) int64 or None[, true, pred][, mask words (B,H,N,ceil(T/32))]);
    true / pred are float32 tensors holding the score-dtype values (pred under autocast with a bias:
    the float32 sums, include/mxa.h score_dtype).  bias: q's dtype, anything that broadcasts to
    (B,H,N,T), read through its strides.  out: the caller's (B,H,N,D) tensor or view of the output
    dtype on q's device, last axis contiguous (a view of a (B,N,H*D) buffer is fine); it is returned.
    elem_bits: 8, or 4 -- Q, K, P and V as MXINT4 and every approximator from the MXINT4 codes
    (the reference at a_elem_format = w_elem_format = "int4"; include/mxa.h mxa_attention_bits:
    float32, no autocast, no ELSA -- the library refuses those).
    One route: mxa_attention_full takes every call its siblings (mxa_attention, _long, _bits) take,
    on the same kernels; which kernel finishes a call is the library's decision."""
    bits = _elem_bits(elem_bits)
    p, dev, (B, H, Nq, T, D), keep = _attn_params(q, k, v, scale, k_top, pred_mode, top_k, approx and top_k, bias,
                                                  flush_subnormals, bfloat, elsa_proj, autocast)
    odt = _out_dtype(q, autocast)
    if out is None:
        out = torch.empty((B, H, Nq, D), dtype=odt, device=dev)
    else:  # the caller's buffer: the kernels store (B, H, N, D) elements through its strides, unchecked
        require_device(q, out)
        if tuple(out.shape) != (B, H, Nq, D):
            raise ValueError(f"out must be {(B, H, Nq, D)} (got {tuple(out.shape)})")
        if out.dtype != odt:
            raise TypeError(f"out must be {odt} (got {out.dtype})")
        if out.stride(3) != 1:
            raise ValueError("out must be contiguous in its last axis")
    _bind_out(p, out)
    idx = _new_idx(p, B, H, Nq, k_top, top_k, dev)
    mask = None
    if return_mask:
        if not top_k:
            raise ValueError("the prune mask exists on the top-k path only")
        mask = torch.empty((B, H, Nq, (T + 31) // 32), dtype=torch.int32, device=dev)
        p.mask_out = mask.data_ptr()
    true_s = pred_s = None
    if return_scores:
        true_s = torch.empty((B, H, Nq, T), dtype=torch.float32, device=dev)
        pred_s = torch.full((B, H, Nq, T), float("nan"), dtype=torch.float32, device=dev)
        p.true_out, p.pred_out = true_s.data_ptr(), pred_s.data_ptr()
    _call_with_workspace(lib().mxa_attention_full_workspace_bytes, lib().mxa_attention_full, "mxa_attention_full", p, bits,
                         dev=dev)
    return (out, idx) + ((true_s, pred_s) if return_scores else ()) + ((mask,) if return_mask else ())


def mx_approx_scores(q: torch.Tensor, k: torch.Tensor, pred_mode: str = "ex_pred",
                     bias: Optional[torch.Tensor] = None, flush_subnormals: bool = False, bfloat: int = 0,
                     elsa_proj: Optional[torch.Tensor] = None, autocast: Optional[torch.dtype] = None,
                     elem_bits: int = 8) -> torch.Tensor:
    """pred = aQ @ aK^T (+ bias) of the approximator `pred_mode` (or ELSA's
    approximation_scores), (B,H,N,T) in the score dtype -- include/mxa.h mxa_approx_scores_bits,
    which takes every call mxa_approx_scores and _long take.  elem_bits 4: the approximators of the
    MXINT4 Q and K.  Float32 q, k under a 16-bit autocast with a bias: float32, as torch promotes the
    reference's `pred + bias`."""
    bits = _elem_bits(elem_bits)
    p, dev, (B, H, Nq, T, D), keep = _attn_params(q, k, None, 1.0, 0, pred_mode, False, True, bias,
                                                  flush_subnormals, bfloat, elsa_proj, autocast)
    pred = torch.empty((B, H, Nq, T), dtype=torch.float32, device=dev)
    p.pred_out = pred.data_ptr()
    _call_with_workspace(lib().mxa_attention_bits_workspace_bytes, lib().mxa_approx_scores_bits, "mxa_approx_scores_bits",
                         p, bits, dev=dev, bad=None)
    odt = _out_dtype(q, autocast)
    if odt == torch.float32 or (bias is not None and q.dtype == torch.float32):
        return pred  # (a 16-bit autocast pred + the float32 bias: torch's promotion, include/mxa.h score_dtype)
    return pred.to(odt)  # the values are exact in odt


class LinearWeightMX:
    """A Linear weight (out_features, in_features) as MXINT8 codes + block exponents
    along in_features on the device (mxa_linear_weight_prep), MFMA-ready in column
    groups of group_width (qkv: the head dim): prepared once, reused by every fused
    call (the weights are constant at inference).  elem_bits 8: MXINT8; 4: MXINT4 (the
    reference's "int4"), which mx_linear / mx_mlp run with the activations at 4 bits too."""

    def __init__(self, weight: torch.Tensor, group_width: int, flush_subnormals: bool = False, bfloat: int = 0,
                 elem_bits: int = 8):
        self.elem_bits = _elem_bits(elem_bits)
        dev = require_device(weight)
        w = _f32(weight.detach(), "weight").contiguous()
        self.out_features, self.in_features = w.shape
        self.group_width = int(group_width)
        nbytes = lib().mxa_linear_weight_bytes_bits(self.out_features, self.in_features, self.group_width,
                                                    self.elem_bits)
        if nbytes < 0:
            raise ValueError(f"group_width {group_width} does not divide out_features {self.out_features}")
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib().mxa_linear_weight_prep_bits(w.data_ptr(), self.out_features, self.in_features, self.group_width,
                                                int(bool(flush_subnormals)), int(bfloat), self.elem_bits,
                                                self.buf.data_ptr(), stream_ptr(dev)), "mxa_linear_weight_prep_bits")
        self.flush, self.bfloat = bool(flush_subnormals), int(bfloat)


def _prepared(weight, group_width: Optional[int] = None, flush_subnormals: bool = False, bfloat: int = 0,
              elem_bits: int = 8) -> "LinearWeightMX":
    """A weight tensor is prepared in groups of group_width (None: one group, its out_features)
    at elem_bits; a LinearWeightMX brings its own groups and width (an explicit non-default
    elem_bits must agree with it)."""
    if isinstance(weight, LinearWeightMX):
        wq = weight
        if int(elem_bits) != 8 and int(elem_bits) != wq.elem_bits:
            raise ValueError(f"the prepared weight has {wq.elem_bits}-bit elements, elem_bits={elem_bits} was asked for")
    else:
        wq = LinearWeightMX(weight, weight.shape[0] if group_width is None else group_width, flush_subnormals, bfloat,
                            elem_bits)
    if (wq.flush, wq.bfloat) != (bool(flush_subnormals), int(bfloat)):
        raise ValueError("the prepared weight was quantized with other flush / bfloat settings")
    return wq


def _rows2d(x: torch.Tensor) -> torch.Tensor:
    """x (..., features) as 2-D rows with unit inner stride (a copy only when it has to be)"""
    x2 = x.reshape(-1, x.shape[-1])
    return x2 if x2.stride(-1) == 1 else x2.contiguous()


def mx_linear(x: torch.Tensor, weight, bias: Optional[torch.Tensor] = None, flush_subnormals: bool = False,
              bfloat: int = 0, autocast: Optional[torch.dtype] = None, elem_bits: int = 8) -> torch.Tensor:
    """mx.Linear forward (microxscaling/mx/linear.py:20-103; include/mxa.h mxa_linear):
    x (..., in_features) float32, weight an (out, in) tensor or a LinearWeightMX (any group
    width); out (..., out) float32 = bf(fl32(MX(x) @ MX(W)^T)) [+ bf(bias)], every product
    the exact sum rounded once.  autocast: the product rounded to float16 / bfloat16 before
    the fp32 bias add (F.linear under torch.autocast).  elem_bits: the width a weight tensor is
    prepared at (8: MXINT8, 4: MXINT4 -- x is quantized at the weight's width)."""
    dev = require_device(x, bias)
    x = _f32(x, "x")
    wq = _prepared(weight, None, flush_subnormals, bfloat, elem_bits)
    if x.shape[-1] != wq.in_features:
        raise ValueError(f"x has {x.shape[-1]} features, the weight {wq.in_features}")
    x2 = _rows2d(x)
    rows = x2.shape[0]
    out = torch.empty((rows, wq.out_features), dtype=torch.float32, device=dev)
    if rows == 0:
        return out.reshape(x.shape[:-1] + (wq.out_features,))
    ac = N.DTYPES[autocast] if autocast is not None and autocast != torch.float32 else 0
    bias = _f32c(bias, "bias")
    ws = _workspace(dev, lib().mxa_linear_workspace_bytes(rows, wq.in_features, wq.out_features))
    check(lib().mxa_linear(x2.data_ptr(), rows, wq.in_features, x2.stride(0), wq.buf.data_ptr(), wq.out_features,
                           _ptr(bias), out.data_ptr(), out.stride(0), int(bool(flush_subnormals)), int(bfloat), ac,
                           ws.data_ptr(), ws.numel(), stream_ptr(dev)), "mxa_linear")
    out = out.reshape(x.shape[:-1] + (wq.out_features,))
    if ac and bias is None:  # F.linear's autocast dtype (the values are already rounded to it)
        out = out.to(autocast)
    return out


def mx_mlp(x: torch.Tensor, w1, b1: Optional[torch.Tensor], w2, b2: Optional[torch.Tensor], act: str = "gelu",
           flush_subnormals: bool = False, bfloat: int = 0, return_hidden: bool = False, elem_bits: int = 8):
    """The MLP of a DeiT / DiT / PixArt block in one call (include/mxa.h mxa_mlp; replaces
    Mlp.forward at inference): y = mx.Linear(gelu(mx.Linear(x; w1, b1)); w2, b2), float32, no
    autocast.  x (..., in); w1 (hidden, in) and w2 (out, hidden) tensors (prepared as one group
    each, as mx_linear does) or LinearWeightMX; act "gelu" (erf) or "gelu_tanh".  fc1 writes
    fc2's MX input codes itself: the fp32 hidden matrix is not materialised.
    return_hidden: (y, pre, act) with pre = fc1's output and act = gelu(pre), (..., hidden).
    elem_bits: as mx_linear; both weights (and x and the hidden codes) have one width."""
    dev = require_device(x, b1, b2)
    x = _f32(x, "x")
    if act not in N.ACTS:
        raise ValueError(f"act must be one of {sorted(N.ACTS)} (got {act!r})")
    wq1 = _prepared(w1, None, flush_subnormals, bfloat, elem_bits)
    wq2 = _prepared(w2, None, flush_subnormals, bfloat, elem_bits)
    if wq1.elem_bits != wq2.elem_bits:
        raise ValueError(f"w1 has {wq1.elem_bits}-bit elements, w2 {wq2.elem_bits}-bit")
    if x.shape[-1] != wq1.in_features:
        raise ValueError(f"x has {x.shape[-1]} features, fc1 takes {wq1.in_features}")
    if wq2.in_features != wq1.out_features:
        raise ValueError(f"fc2 takes {wq2.in_features} features, fc1 gives {wq1.out_features}")
    hidden, outf = wq1.out_features, wq2.out_features
    x2 = _rows2d(x)
    rows = x2.shape[0]
    y = torch.empty((rows, outf), dtype=torch.float32, device=dev)
    pre = torch.empty((rows, hidden), dtype=torch.float32, device=dev) if return_hidden else None
    actv = torch.empty((rows, hidden), dtype=torch.float32, device=dev) if return_hidden else None
    if rows:
        b1, b2 = _f32c(b1, "b1"), _f32c(b2, "b2")
        nbytes = lib().mxa_mlp_workspace_bytes(rows, wq1.in_features, wq1.buf.data_ptr(), hidden, outf)
        if nbytes < 0:
            raise ValueError("mxa_mlp_workspace_bytes: bad shape")
        ws = _workspace(dev, nbytes)
        check(lib().mxa_mlp(x2.data_ptr(), rows, wq1.in_features, x2.stride(0), wq1.buf.data_ptr(), hidden,
                            _ptr(b1), N.ACTS[act], wq2.buf.data_ptr(), outf, _ptr(b2), y.data_ptr(), y.stride(0),
                            _ptr(pre), _ptr(actv),
                            int(bool(flush_subnormals)), int(bfloat), ws.data_ptr(), ws.numel(), stream_ptr(dev)),
              "mxa_mlp")
    y = y.reshape(x.shape[:-1] + (outf,))
    if return_hidden:
        return y, pre.reshape(x.shape[:-1] + (hidden,)), actv.reshape(x.shape[:-1] + (hidden,))
    return y


def _fused_entry(name: str, bits: int):
    """(size function, entry point, its name, trailing arguments) of the fused block `name` at a width:
    8 the entry point itself (today's call), 4 its *_bits form with the width behind the structs."""
    if bits == 8:
        return getattr(lib(), name + "_workspace_bytes"), getattr(lib(), name), name, ()
    return getattr(lib(), name + "_bits_workspace_bytes"), getattr(lib(), name + "_bits"), name + "_bits", (bits,)


def _self_block_entry(name: str, bits: int, keys: int):
    """_fused_entry of a self-attention block on rows of `keys` keys: up to 512 today's call; over 512 the
    *_full form at either width (include/mxa.h mxa_qkv_attention_full: rows of 513 .. 1,024 keys)."""
    if keys <= 512:
        return _fused_entry(name, bits)
    return getattr(lib(), name + "_full_workspace_bytes"), getattr(lib(), name + "_full"), name + "_full", (bits,)


def _proj_params(proj_weight, proj_bias, C: int, rows: int, flush_subnormals: bool, bfloat: int, dev,
                 elem_bits: int = 8):
    """(ProjParams, y (rows, out_features), keep) for the proj Linear behind the attention."""
    wp = _prepared(proj_weight, None, flush_subnormals, bfloat, elem_bits)
    if wp.in_features != C:
        raise ValueError(f"proj weight takes {wp.in_features} features, the attention gives H*D = {C}")
    pj = N.ProjParams()
    pj.wq, pj.out_features = wp.buf.data_ptr(), wp.out_features
    pb = _f32c(proj_bias, "proj_bias")
    pj.bias = _ptr(pb)
    keep = [wp, pb]
    y = torch.empty((rows, wp.out_features), dtype=torch.float32, device=dev)
    pj.y, pj.y_row_stride = y.data_ptr(), y.stride(0)
    return pj, y, keep


def mx_topk_attention_proj(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float, proj_weight,
                           proj_bias: Optional[torch.Tensor] = None, k_top: int = 20, pred_mode: str = "ex_pred",
                           approx: bool = True, bias: Optional[torch.Tensor] = None, flush_subnormals: bool = False,
                           bfloat: int = 0, elsa_proj: Optional[torch.Tensor] = None, elem_bits: int = 8):
    """The top-k attention core with the proj mx.Linear fused behind it (include/mxa.h
    mxa_attention_proj): y = proj(out.transpose(1, 2).reshape(B, N, H*D)) as (B, N, out)
    float32, plus idx (B,H,N,k).  float32 q, k, v (views fine).
    elem_bits 4 (W4A4, mxa_attention_proj_bits): the attention of mx_topk_attention(elem_bits=4) and
    the proj at MXINT4 -- a weight tensor is prepared at 4 bits, a LinearWeightMX must be a 4-bit one.
    Rows of 513 .. 1,024 keys: mxa_attention_proj_full at either width, every k_top <= T."""
    bits = _elem_bits(elem_bits)
    p, dev, (B, H, Nq, T, D), keep = _attn_params(q, k, v, scale, k_top, pred_mode, True, approx, bias,
                                                  flush_subnormals, bfloat, elsa_proj)
    if p.dtype != N.DT_F32:
        raise TypeError("the fused proj takes float32 q, k, v")
    idx = _new_idx(p, B, H, Nq, k_top, True, dev)
    pj, y, keep2 = _proj_params(proj_weight, proj_bias, H * D, B * Nq, flush_subnormals, bfloat, dev, bits)
    size_fn, fn, name, tail = _self_block_entry("mxa_attention_proj", bits, T)
    _call_with_workspace(size_fn, fn, name, p, None, ctypes.byref(pj), *tail, dev=dev)
    return y.reshape(B, Nq, -1), idx


def _check_fits(wq: "LinearWeightMX", name: str, in_features: int, D: int, out_features: int, want: str):
    """a fused projection's prepared weight: its features, head-dim groups and rows"""
    if wq.in_features != in_features or wq.group_width != D or wq.out_features != out_features:
        raise ValueError(f"{name} ({wq.out_features}, {wq.in_features}) / group {wq.group_width} does not fit {want}")


def mx_qkv_attention(x: torch.Tensor, weight, bias: Optional[torch.Tensor], num_heads: int, scale: float,
                     k_top: int = 20, pred_mode: str = "ex_pred", top_k: bool = True, approx: bool = True,
                     flush_subnormals: bool = False, bfloat: int = 0, return_qkv: bool = False,
                     elsa_proj: Optional[torch.Tensor] = None, autocast: Optional[torch.dtype] = None,
                     proj_weight=None, proj_bias: Optional[torch.Tensor] = None, elem_bits: int = 8,
                     attn_bias: Optional[torch.Tensor] = None):
    """The qkv mx.Linear fused into the attention core (include/mxa.h mxa_qkv_attention):
    x (B, N, C) float32 tokens; weight a (3C', C) tensor or a LinearWeightMX; returns
    (out (B,H,N,D), idx (B,H,N,k) or None[, qkv (B,N,3C') fp32 projection]).
    bias is the Linear's; attn_bias the additive score bias, float32, broadcast to (B, H, N, N) as
    mx_topk_attention's.
    autocast (float16 / bfloat16): torch.autocast around the module -- the projection's
    product is rounded to it before the fp32 bias add, and the attention's matmuls return
    it (the output is of that dtype).
    elem_bits 4 (W4A4, mxa_qkv_attention_bits / mxa_attention_proj_bits): x, the weights, Q, K, P, V
    and the proj's input at MXINT4 -- weight tensors are prepared at 4 bits, a LinearWeightMX must be a
    4-bit one; float32, no autocast.
    More than 512 tokens (up to 1,024: PixArt / DiT at 512 x 512, DeiT at 384 x 384): mxa_qkv_attention_full /
    mxa_attention_proj_full at either width -- everything mx_topk_attention serves on such rows, the dense
    branch without the proj; autocast there raises NativeError (status -2)."""
    bits = _elem_bits(elem_bits)
    if bits == 4 and autocast not in (None, torch.float32):
        raise ValueError("elem_bits=4 runs in float32: no autocast")
    dev = require_device(x, bias, elsa_proj, attn_bias)
    xs = _token_rows(x, "x", "N")
    B, Ntok, C = x.shape
    out_f = weight.out_features if isinstance(weight, LinearWeightMX) else weight.shape[0]
    if out_f % (3 * num_heads):
        raise ValueError(f"weight rows {out_f} are not 3 * heads * head_dim")
    D = out_f // (3 * num_heads)
    wq = _prepared(weight, D, flush_subnormals, bfloat, bits)
    _check_fits(wq, "weight", C, D, out_f, f"x C={C}, heads={num_heads}")
    # q / k / v are produced inside the call
    p, keep = _attn_shape_params(dev, torch.float32, B, num_heads, Ntok, Ntok, D, scale, k_top, pred_mode, top_k,
                                 approx and top_k, attn_bias, flush_subnormals, bfloat, elsa_proj, autocast)
    out = _bind_out(p, torch.empty((B, num_heads, Ntok, D), dtype=_out_dtype(x, autocast), device=dev))
    idx = _new_idx(p, B, num_heads, Ntok, k_top, top_k, dev)
    xp = N.QkvParams()
    xp.x, xp.x_row_stride, xp.C, xp.wq = x.data_ptr(), xs, C, wq.buf.data_ptr()
    xp.autocast_dtype = p.score_dtype
    bias = _f32c(bias, "bias")
    qkv = torch.empty((B, Ntok, wq.out_features), dtype=torch.float32, device=dev) if return_qkv else None
    xp.bias, xp.qkv_out = _ptr(bias), _ptr(qkv)
    if proj_weight is not None:
        # ... then the proj mx.Linear on the attention output (mxa_attention_proj): (y, idx[, qkv])
        if not top_k or autocast not in (None, torch.float32):
            raise ValueError("the fused proj runs on the float32 top-k path")
        pj, y, keep2 = _proj_params(proj_weight, proj_bias, num_heads * D, B * Ntok, flush_subnormals, bfloat, dev, bits)
        p.out = None
        size_fn, fn, name, tail = _self_block_entry("mxa_attention_proj", bits, Ntok)
        _call_with_workspace(size_fn, fn, name, p, ctypes.byref(xp), ctypes.byref(pj), *tail, dev=dev, bad="bad shape")
        y = y.reshape(B, Ntok, -1)
        return (y, idx, qkv) if return_qkv else (y, idx)
    size_fn, fn, name, tail = _self_block_entry("mxa_qkv_attention", bits, Ntok)
    _call_with_workspace(size_fn, fn, name, p, ctypes.byref(xp), *tail, dev=dev, bad="bad shape")
    return (out, idx, qkv) if return_qkv else (out, idx)


def _token_rows(t: torch.Tensor, name: str, rows: str = "rows"):
    """(B, rows, C) float32 tokens with contiguous C and evenly strided rows -> the row stride"""
    t = _f32(t, name)
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{name} must be (B, {rows}, C) with contiguous C")
    if t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1):
        raise ValueError(f"{name} rows must be evenly strided over (B, {rows})")
    return t.stride(1)


def mx_cross_attention(x: torch.Tensor, cond: torch.Tensor, q_weight, q_bias: Optional[torch.Tensor], kv_weight,
                       kv_bias: Optional[torch.Tensor], num_heads: int, scale: float, k_top: int = 20,
                       pred_mode: str = "ex_pred", top_k: bool = True, approx: bool = True,
                       bias: Optional[torch.Tensor] = None, flush_subnormals: bool = False, bfloat: int = 0,
                       return_proj: bool = False, proj_weight=None, proj_bias: Optional[torch.Tensor] = None,
                       elem_bits: int = 8):
    """Cross-attention with its q and kv mx.Linears fused in front (include/mxa.h
    mxa_cross_attention; PixArt's MXCrossAttention.forward): x (B, N, C) float32 query tokens,
    cond (B, T, C_kv) float32 key / value tokens; q_weight (H*D, C) and kv_weight
    = cat([W_k, W_v]) (2*H*D, C_kv), tensors or LinearWeightMX of group width D; bias the
    additive mask, broadcast to (B, H, N, T).  Returns (out (B,H,N,D), idx (B,H,N,k) or None);
    with proj_weight the proj mx.Linear runs behind the attention and y (B, N, out_features)
    takes out's place (top-k only); return_proj appends the fp32 projections q (B, N, H*D) and
    kv (B, T, 2*H*D).  Float32, no autocast.
    elem_bits 4 (W4A4, mxa_cross_attention_bits): x, cond, the weights, Q, K, P, V and the proj's input
    at MXINT4 -- weight tensors are prepared at 4 bits, a LinearWeightMX must be a 4-bit one."""
    bits = _elem_bits(elem_bits)
    dev = require_device(x, cond, q_bias, kv_bias, bias)
    xs, cs = _token_rows(x, "x"), _token_rows(cond, "cond")
    B, Ntok, C = x.shape
    Bc, T, Ckv = cond.shape
    if Bc != B:
        raise ValueError(f"x has {B} images, cond {Bc}")
    HD = q_weight.out_features if isinstance(q_weight, LinearWeightMX) else q_weight.shape[0]
    if HD % num_heads:
        raise ValueError(f"q weight rows {HD} are not heads * head_dim")
    D = HD // num_heads
    wq = _prepared(q_weight, D, flush_subnormals, bfloat, bits)
    wkv = _prepared(kv_weight, D, flush_subnormals, bfloat, bits)
    _check_fits(wq, "q weight", C, D, HD, f"x C={C}, heads={num_heads}")
    _check_fits(wkv, "kv weight", Ckv, D, 2 * HD, f"cond C_kv={Ckv}, 2 * heads * head_dim = {2 * HD}")
    # q / k / v are produced inside the call
    p, keep = _attn_shape_params(dev, torch.float32, B, num_heads, Ntok, T, D, scale, k_top, pred_mode, top_k,
                                 approx and top_k, bias, flush_subnormals, bfloat, None)
    idx = _new_idx(p, B, num_heads, Ntok, k_top, top_k, dev)
    xc = N.CrossParams()
    xc.x, xc.x_row_stride, xc.C = x.data_ptr(), xs, C
    xc.cond, xc.cond_row_stride, xc.C_kv = cond.data_ptr(), cs, Ckv
    xc.wq_q, xc.wq_kv = wq.buf.data_ptr(), wkv.buf.data_ptr()
    q_bias, kv_bias = _f32c(q_bias, "q_bias"), _f32c(kv_bias, "kv_bias")
    xc.bias_q, xc.bias_kv = _ptr(q_bias), _ptr(kv_bias)
    qo = kvo = None
    if return_proj:
        qo = torch.empty((B, Ntok, HD), dtype=torch.float32, device=dev)
        kvo = torch.empty((B, T, 2 * HD), dtype=torch.float32, device=dev)
        xc.q_out, xc.kv_out = qo.data_ptr(), kvo.data_ptr()
    pj = None
    if proj_weight is not None:
        if not top_k:
            raise ValueError("the fused proj runs on the top-k path")
        pj, y, keep2 = _proj_params(proj_weight, proj_bias, HD, B * Ntok, flush_subnormals, bfloat, dev, bits)
        res = y.reshape(B, Ntok, -1)
    else:
        res = _bind_out(p, torch.empty((B, num_heads, Ntok, D), dtype=torch.float32, device=dev))
    size_fn, fn, name, tail = _fused_entry("mxa_cross_attention", bits)
    _call_with_workspace(size_fn, fn, name, p, ctypes.byref(xc), ctypes.byref(pj) if pj is not None else None, *tail,
                         dev=dev, bad="bad shape")
    return (res, idx, qo, kvo) if return_proj else (res, idx)


def selftest_mfma(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    dev = require_device(a, b)
    c = torch.empty((16, 16), dtype=torch.int32, device=dev)
    check(lib().mxa_selftest_mfma(a.contiguous().data_ptr(), b.contiguous().data_ptr(), c.data_ptr(),
                                  stream_ptr(dev)), "mxa_selftest_mfma")
    return c


def selftest_mfma32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """C = A (32x32 int8) @ B (32x32 int8) by one v_mfma_i32_32x32x32_i8 through the
    finishing kernel's lane maps."""
    dev = require_device(a, b)
    c = torch.empty((32, 32), dtype=torch.int32, device=dev)
    check(lib().mxa_selftest_mfma32(a.contiguous().data_ptr(), b.contiguous().data_ptr(), c.data_ptr(),
                                    stream_ptr(dev)), "mxa_selftest_mfma32")
    return c
